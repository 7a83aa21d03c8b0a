"""The lidar noise of npa_world_scan_noisy (include/neupan_amd.h) restated for tests/test_scan_noise*.py: the counter-based
generator in Python integers, the Box-Muller transform in `math`, and a noisy scan built on the cast of tests/world_ref.py.

    z = mix(mix(mix(mix(seed + scene) + beam) + draw) + k),  U = (z >> 11) 2^-53
    g(k0) = sqrt(-2 ln(1 - U(k0))) cos(2 pi U(k0 + 1)),  g_a = g(0),  g_r = g(2)
    beam i is cast along ang_i + angle_std g_a; a hit reports min(max(t + std g_r, 0) + 0, range_max), a miss range_max
"""
from math import cos, log, pi, sin, sqrt

import numpy as np

import world_ref as wr
from oracle import frontend_oracle as fo

M64 = (1 << 64) - 1


def mix(z):
    """the splitmix64 finaliser of npa_world_behave"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniform(seed, scene, beam, draw, k):
    z = mix((int(seed) + int(scene)) & M64)
    for c in (beam, draw, k):
        z = mix((z + int(c)) & M64)
    return float(z >> 11) * 2.0 ** -53


def gauss(seed, scene, beam, draw, k0):
    u0, u1 = uniform(seed, scene, beam, draw, k0), uniform(seed, scene, beam, draw, k0 + 1)
    return sqrt(-2.0 * log(1.0 - u0)) * cos((2.0 * pi) * u1)


def draws(seed, scene, draw, first_beam, n):
    """(n, 2): (g_a, g_r) of the beams first_beam .. first_beam + n - 1"""
    return np.array([[gauss(seed, scene, i, draw, 0), gauss(seed, scene, i, draw, 2)] for i in range(first_beam, first_beam + n)],
                    dtype=np.float64).reshape(n, 2)


def cast(circles, segments, state, angles, range_max, offset=(0.0, 0.0, 0.0), skip=None):
    """world_ref.scan along the beam angles `angles` (sensor frame) instead of a linspace: its cast, its tie rule, its `ill`.
    world_ref.scan takes its directions from world_ref.beam_directions; for the length of the call that name gives the
    directions of `angles`, composed exactly as beam_directions composes them."""
    o, (sc, ss), (rc, rs) = wr.sensor_pose(state, offset)
    lx, ly = np.array([cos(a) for a in angles]), np.array([sin(a) for a in angles])
    tx, ty = sc * lx + (-ss) * ly, ss * lx + sc * ly
    d = np.stack([rc * tx + (-rs) * ty, rs * tx + rc * ty], axis=1)
    keep = wr.beam_directions
    wr.beam_directions = lambda *a, **k: (o, d)
    try:
        return wr.scan(circles, segments, state, len(angles), 0.0, 0.0, range_max, offset=offset, skip=skip)
    finally:
        wr.beam_directions = keep


def scan(circles, segments, state, n, angle_min, angle_max, range_max, std, angle_std, seed=0, scene=0, draw=0,
         offset=(0.0, 0.0, 0.0), skip=None):
    """dict(ranges, hit, vel, ill, g (n, 2), clamped (n,) bool) of the noisy scan.  `ill` is the cast's, extended by the hit
    beams whose unclamped t + std g_r lies within 1e-6 of 0 or of range_max (there the clamp decides within rounding)."""
    g = draws(seed, scene, draw, 0, n)
    ang = fo._linspace(angle_min, angle_max, n)
    ref = cast(circles, segments, state, ang + angle_std * g[:, 0], range_max, offset, skip)
    hit = ref["hit"] >= 0
    raw = ref["ranges"] + std * g[:, 1]
    ranges = np.where(hit, np.minimum(np.maximum(raw, 0.0) + 0.0, float(range_max)), float(range_max))
    ill = ref["ill"] | (hit & ((np.abs(raw) < 1e-6) | (np.abs(raw - range_max) < 1e-6)))
    return dict(ranges=ranges, hit=ref["hit"], vel=ref["vel"], ill=ill, g=g, clamped=hit & ((raw <= 0.0) | (raw >= range_max)))


# ---------------------------------------------------------------------------------------------------- the GPU test's inputs
STD, ANGLE_STD, SEED, RMAX, BEAMS = 0.2, 0.02, 11, 10.0, (100, 257)
_INPUTS, _REF = [], {}


def inputs():
    """tests/test_world_gpu.py's 8 random worlds and 4 poses in each (made once)"""
    if not _INPUTS:
        from test_world_gpu import random_world
        rng = np.random.default_rng(0)
        ws = [random_world(rng) for _ in range(8)]
        poses = np.concatenate([rng.uniform(-8, 8, (8, 4, 2)), rng.uniform(-pi, pi, (8, 4, 1))], axis=2)
        _INPUTS.extend([ws, poses])
    return _INPUTS


def ref_scan(k, p, n):
    """the noisy restatement of world k seen from its pose p (scene p of the generator, draw 0) with n beams over (-pi, pi):
    computed once, shared by the CPU and the GPU test, never written to"""
    if (k, p, n) not in _REF:
        ws, poses = inputs()
        _REF[k, p, n] = scan(ws[k][0], ws[k][1], poses[k, p], n, -pi, pi, RMAX, STD, ANGLE_STD, seed=SEED, scene=p, draw=0)
    return _REF[k, p, n]
