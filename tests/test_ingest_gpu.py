"""GPU tests of the host-fed input path: npa_ingest_unpack (csrc/ingest.hip) against the record format restated in numpy,
its containment of malformed headers, and neupan_amd.ingest.InputPipeline against the resident prepared step."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_helpers import make_gpu_pan
from helpers import CONFIGS

pytestmark = pytest.mark.gpu

T, N_STRIDE = 10, 130
N_B = (0, 1, 63, 64, 65, 130)       # empty, one point, either side of one wave, the full stride: clouds start at unaligned words
SENTINEL = np.float32(12345.0)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def packed_record(B, vel, seed=11):
    from neupan_amd.ingest import HostRecord, RecordLayout
    lay = RecordLayout(B, T, N_STRIDE, vel)
    rec = HostRecord(lay)
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    ns = N_B[-B:] if B > 1 else (65,)
    src = dict(nom_s=f(B, 3, T + 1), nom_u=f(B, 2, T), ref_s=f(B, 3, T + 1), ref_us=f(B, T), n=ns,
               clouds=[f(2, n) for n in ns], vels=[f(2, n) for n in ns] if vel else None)
    rec.pack(src["nom_s"], src["nom_u"], src["ref_s"], src["ref_us"], src["clouds"], src["vels"])
    return lay, rec, src


def run_unpack(lay, words, record_bytes, alloc_words=None, fill=None):
    """Upload `words` into a device buffer (alloc_words long, the rest = fill) and unpack it into NaN-filled tensors."""
    from neupan_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B = lay.batch
    buf = np.full(alloc_words or words.size, 0, dtype=np.int32)
    if fill is not None:
        buf.view(np.float32)[:] = fill
    buf[:record_bytes // 4] = words[:record_bytes // 4]
    d_rec = torch.from_numpy(buf).to(dev)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    out = dict(nom_s=nan(B, 3, T + 1), nom_u=nan(B, 2, T), ref_s=nan(B, 3, T + 1), ref_us=nan(B, T), points=nan(B, 2, N_STRIDE),
               velocities=nan(B, 2, N_STRIDE) if lay.velocities else None,
               n_points=torch.full((B,), -7, dtype=torch.int32, device=dev),
               status=torch.tensor([0, 2 ** 31 - 1], dtype=torch.int32, device=dev))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = lib.npa_ingest_unpack(B, T, N_STRIDE, int(lay.velocities), p(d_rec), record_bytes, p(out["nom_s"]), p(out["nom_u"]),
                               p(out["ref_s"]), p(out["ref_us"]), p(out["points"]), p(out["velocities"]), p(out["n_points"]),
                               p(out["status"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, lib.npa_last_error()
    torch.cuda.synchronize(dev)
    return out


def check_scene(out, src, b, vel):
    n = src["n"][b]
    nan_bits = bits(np.full(1, np.nan, dtype=np.float32))[0]
    assert np.array_equal(bits(out["points"][b, :, :n]), bits(src["clouds"][b]))
    assert (bits(out["points"][b, :, n:]) == nan_bits).all()             # columns beyond n_b are not written
    if vel:
        assert np.array_equal(bits(out["velocities"][b, :, :n]), bits(src["vels"][b]))
        assert (bits(out["velocities"][b, :, n:]) == nan_bits).all()


@pytest.mark.parametrize("B", [6, 1])
@pytest.mark.parametrize("vel", [False, True])
def test_unpack_matches_numpy_bitwise(B, vel):
    lay, rec, src = packed_record(B, vel)
    out = run_unpack(lay, rec.words, rec.used_bytes)
    for k in ("nom_s", "nom_u", "ref_s", "ref_us"):
        assert np.array_equal(bits(out[k]), bits(src[k])), k
    assert out["n_points"].cpu().tolist() == list(src["n"])
    for b in range(B):
        check_scene(out, src, b, vel)
    assert out["status"].cpu().tolist() == [0, 2 ** 31 - 1]
    if B == 6:      # this shape takes both copy paths: 16-byte accesses where source and destination allow, 4-byte ones elsewhere
        wide = {(int(rec.cloud_off[b]) + c * n) % 4 == 0 and ((2 * b + (c & 1)) * N_STRIDE) % 4 == 0
                for b, n in enumerate(src["n"]) if n >= 4 for c in range(lay.comps)}
        assert wide == {True, False}


def test_selection_never_reads_beyond_n_points():
    """The unpack leaves columns [n_b, n_stride) of the padded cloud alone, so whatever an earlier cycle left there stays:
    a plan must not depend on it.  NaN there against zeros there, bitwise."""
    from neupan_amd.scenes import make_batch
    cfg = CONFIGS["corridor_diff_small"]
    B, N = 4, cfg.n_points
    pan = make_gpu_pan(cfg)
    b = make_batch(cfg, 0, B)
    n_b = np.array([0, 1, 77, 150], dtype=np.int32)
    outs = []
    for tail in (np.nan, 0.0):
        pts = b["points"].copy()
        for s in range(B):
            pts[s, :, n_b[s]:] = tail
        o = pan.forward_batch(b["nom_s"], b["nom_u"], b["ref_s"], b["ref_us"], pts, None, n_b, reset_state=True)
        torch.cuda.synchronize()
        outs.append({k: v.clone() for k, v in o.items() if v is not None})
    for k in ("opt_s", "opt_u", "min_distance", "iters"):
        assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), k
    for k in ("opt_d", "nrmp_points"):             # (scene 0 has no points: nothing defines its rows)
        assert np.array_equal(bits(outs[0][k][1:]), bits(outs[1][k][1:])), k
    assert torch.isfinite(outs[0]["opt_u"]).all()


@pytest.mark.parametrize("vel", [False, True])
def test_malformed_records_are_contained(vel):
    """Three scenes lie about their cloud; the record sits in the first half of an allocation whose second half is a
    sentinel, so an offset taken on trust would read sentinels (inside the allocation) and show them."""
    B = 6
    lay, rec, src = packed_record(B, vel)
    used = rec.used_bytes
    rec.n_points[2] = N_STRIDE + 1                       # longer than the stride
    rec.n_points[4] = -1                                 # negative
    rec.cloud_off[5] = (used - lay.offsets["cloud"]) // 4 + 8      # points past record_bytes (n = 130 stays)
    total_words = lay.total_bytes // 4
    out = run_unpack(lay, rec.words, used, alloc_words=2 * total_words, fill=SENTINEL)
    assert out["n_points"].cpu().tolist() == [0, 1, 0, 64, 0, 0]
    assert out["status"].cpu().tolist() == [3, 2]
    for k in ("nom_s", "nom_u", "ref_s", "ref_us"):
        assert np.array_equal(bits(out[k]), bits(src[k])), k
    for b in (0, 1, 3):
        check_scene(out, src, b, vel)
    s_bits = bits(np.full(1, SENTINEL))[0]
    for k in ("nom_s", "nom_u", "ref_s", "ref_us", "points", "velocities"):
        if out[k] is not None:
            assert not (bits(out[k]) == s_bits).any(), k
    # a scene whose cloud ends exactly at record_bytes is fine; one word further is not
    lay, rec, src = packed_record(B, vel)
    out = run_unpack(lay, rec.words, rec.used_bytes - 4, alloc_words=2 * total_words, fill=SENTINEL)
    assert out["n_points"].cpu().tolist() == [0, 1, 63, 64, 65, 0] and out["status"].cpu().tolist() == [1, 5]


def cycle_inputs(cfg, B, c):
    """Cycle c of a B-robot fleet: fresh scenes, clouds of other lengths every cycle (50 .. the stride)."""
    from neupan_amd.scenes import make_scene
    rng = np.random.default_rng(100 + c)
    n = [int(v) for v in rng.integers(50, cfg.n_points + 1, B)]
    if c == 2:
        n[1] = 0
    sc = [make_scene(cfg, 1000 + 10 * c + b, n_points=max(n[b], 1)) for b in range(B)]
    st = lambda k: np.stack([s[k] for s in sc])
    return dict(nom_s=st("nom_s"), nom_u=st("nom_u"), ref_s=st("ref_s"), ref_us=st("ref_us"),
                clouds=[sc[b]["points"][:, :n[b]] for b in range(B)], n=np.array(n, dtype=np.int32))


KEYS = ("opt_u", "opt_s", "min_distance", "iters")


def same(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in KEYS)


@pytest.fixture(scope="module")
def resident_cycles():
    """Planner A, once for both depths: a resident prepared step refreshed with copy_() and a host synchronisation per cycle,
    state carried across the six cycles (primed on cycle 0's inputs)."""
    cfg = CONFIGS["corridor_diff_small"]
    B, N, dev = 4, cfg.n_points, torch.device("cuda:0")
    cyc = [cycle_inputs(cfg, B, c) for c in range(6)]
    pan = make_gpu_pan(cfg)

    def padded(ci):
        p = np.zeros((B, 2, N), dtype=np.float32)
        for b in range(B):
            p[b, :, :ci["n"][b]] = ci["clouds"][b]
        return p
    t = {k: torch.from_numpy(cyc[0][k]).to(dev) for k in ("nom_s", "nom_u", "ref_s", "ref_us")}
    t["points"], t["n"] = torch.from_numpy(padded(cyc[0])).to(dev), torch.from_numpy(cyc[0]["n"]).to(dev)
    step = pan.make_step(t["nom_s"], t["nom_u"], t["ref_s"], t["ref_us"], t["points"], None, t["n"], reset_state=True)
    outs = []
    for ci in cyc:
        for k in ("nom_s", "nom_u", "ref_s", "ref_us"):
            t[k].copy_(torch.from_numpy(ci[k]))
        t["points"].copy_(torch.from_numpy(padded(ci)))
        t["n"].copy_(torch.from_numpy(ci["n"]))
        torch.cuda.synchronize()
        o = step()
        torch.cuda.synchronize()
        outs.append({k: o[k].clone() for k in KEYS})
    return cfg, B, cyc, outs


@pytest.mark.parametrize("depth", [2, 1])
def test_pipeline_equals_resident_path_over_cycles(resident_cycles, depth):
    from neupan_amd.ingest import InputPipeline
    cfg, B, cyc, want = resident_cycles
    pan = make_gpu_pan(cfg)
    pipe = InputPipeline(pan, B, cfg.n_points, depth=depth)

    def feed(ci):
        rec = pipe.acquire()
        rec.words[:] = 0x7FC0DEAD                       # whatever the record held is gone the moment it is handed back
        rec.pack(ci["nom_s"], ci["nom_u"], ci["ref_s"], ci["ref_us"], ci["clouds"])
        assert pipe.submit(rec) == pipe.layout.offsets["cloud"] + 8 * int(ci["n"].sum())
    feed(cyc[0])
    step = pipe.make_step(reset_state=True)             # primes on cycle 0, like planner A
    got = []
    feed(cyc[0])
    for c in range(6):                                  # no host synchronisation in here
        if depth > 1 and c + 1 < 6:
            feed(cyc[c + 1])                            # the next cycle's upload is on its way before this one is planned
        o = step()
        got.append({k: o[k].clone() for k in KEYS})
        if depth == 1 and c + 1 < 6:
            feed(cyc[c + 1])
    assert pipe.status() == (0, -1)
    for c in range(6):
        assert same(got[c], want[c]), f"cycle {c}"
    assert not same(want[0], want[1])                   # (the cycles do differ)
    with pytest.raises(Exception, match="submitted record"):
        step()                                          # nothing submitted: refused, not planned on stale inputs
    with pytest.raises(Exception, match="graph"):
        InputPipeline(pan, B, cfg.n_points).make_step(graph=True)


def test_pipelined_steps_in_a_merged_chain():
    """Two pipelines feed two steps that share ONE stream; issued through StepGroup (pre_issue runs under the member's
    stream) they give what the same steps give issued one after the other."""
    from neupan_amd.ingest import InputPipeline
    from neupan_amd.pan import StepGroup
    cfg = CONFIGS["corridor_diff_small"]
    B, dev = 4, torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    pans = [make_gpu_pan(cfg) for _ in range(2)]
    pipes = [InputPipeline(p, B, cfg.n_points) for p in pans]
    cyc = [cycle_inputs(cfg, B, 3 + j) for j in range(2)]

    def feed(j):
        rec, ci = pipes[j].acquire(), cyc[j]
        rec.pack(ci["nom_s"], ci["nom_u"], ci["ref_s"], ci["ref_us"], ci["clouds"])
        pipes[j].submit(rec)
    with torch.cuda.stream(st):
        steps = [p.make_step(reset_every_step=True) for p in pipes]     # every step the same work: state cleared per step
        feed(0); feed(1)
        one = []
        for s in steps:
            o = s()                                                     # (one record per call)
            one.append({k: o[k].clone() for k in KEYS})
    torch.cuda.synchronize()
    group = StepGroup(steps, [st, st])
    feed(0); feed(1)
    res = group.issue()
    torch.cuda.synchronize()
    print("merged launches:", group.merged())
    for j in range(2):
        assert same(res[j], one[j]), j
    assert not same(one[0], one[1])
    assert all(p.status() == (0, -1) for p in pipes)
