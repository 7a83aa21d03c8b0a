"""The three launches of csrc/lon.hip restated in numpy, and the scenario tables of the LON tests.

The kernels do single IEEE operations in a stated order (include/neupan_amd.h: npa_lon_loss, npa_lon_chain, npa_lon_adam), and
numpy's float32 / float64 scalars and arrays do the same, one rounding per operator -- so these are bit-for-bit restatements and
the tests compare with array_equal.  Parameter-shaped arrays are rows of 8: q_s[0..2], p_u, eta, d_max, d_min, reserved."""
import numpy as np

f32, f64 = np.float32, np.float64


def loss(state, last_xy, opt_d, min_distance, stop, arrived, collided, stuck_count, ended, override, threshold,
         stuck_threshold=0.01, stuck_patience=5, weight=10.0, offset=50.0):
    """npa_lon_loss -> dict(active, loss, stuck, ended, stuck_count, last_xy, override, grad_s, grad_u, grad_d); the inputs are
    not modified"""
    state, last_xy = np.asarray(state, dtype=f64), np.asarray(last_xy, dtype=f64)
    d = np.asarray(opt_d, dtype=f32)
    B, T = d.shape
    was = np.asarray(ended) != 0
    dx, dy = state[:, 0] - last_xy[:, 0], state[:, 1] - last_xy[:, 1]
    disp = np.sqrt(dx * dx + dy * dy)
    count = np.where(was, stuck_count, np.asarray(stuck_count) + (disp < f64(stuck_threshold))).astype(np.int32)
    stuck = count > int(stuck_patience)
    S = np.zeros(B, dtype=f32)
    for t in range(T):
        S = S + d[:, t]                                       # first to last, one float32 addition each
    w, off = f32(weight), f32(offset)
    hit = np.asarray(min_distance, dtype=f32) <= f32(threshold)
    fire_hit, fire_stuck = ~was & hit, ~was & ~hit & stuck
    zero = np.zeros(B, dtype=f32)
    l = np.where(fire_hit, w * (off - S), np.where(fire_stuck, w * (off + S), zero)).astype(f32)
    g = np.where(fire_hit, -w, np.where(fire_stuck, w, f32(0))).astype(f32)
    end = was | (np.asarray(arrived) != 0) | (np.asarray(collided) != 0) | (np.asarray(stop) != 0) | stuck
    ov = np.where(end[:, None], f32(0), np.asarray(override, dtype=f32)).astype(f32)
    return dict(active=(~was).astype(np.int32), loss=l, stuck=stuck, ended=end.astype(np.int32), stuck_count=count,
                last_xy=state[:, :2].copy(), override=ov, grad_s=np.zeros((B, 3, T + 1), dtype=f32),
                grad_u=np.zeros((B, 2, T), dtype=f32), grad_d=np.repeat(g[:, None], T, axis=1))


def chain(k, iters, grad_theta, grad_nom_s, tot, gs, gu, gd, bad):
    """npa_lon_chain -> (tot, gs, gu, gd, bad) after the call"""
    ran = np.asarray(iters) > k
    gt = np.asarray(grad_theta, dtype=f32)
    tot = np.array(tot, dtype=f64)
    tot[:, :7] = np.where(ran[:, None], tot[:, :7] + gt[:, :7].astype(f64), tot[:, :7])
    gs = np.where(ran[:, None, None], np.asarray(grad_nom_s, dtype=f32), gs).astype(f32)
    gu = np.where(ran[:, None, None], f32(0), gu).astype(f32)
    gd = np.where(ran[:, None], f32(0), gd).astype(f32)
    bad = (np.asarray(bad) + (ran & (gt[:, 7] != 0))).astype(np.int32)
    return tot, gs, gu, gd, bad


def adam_scalars(t, lr=5e-3, betas=(0.9, 0.999), eps=1e-8):
    """the by-value scalars of step t, computed in double as torch.optim.Adam computes them, then float32 (the ABI's type)"""
    b1, b2 = float(betas[0]), float(betas[1])
    return tuple(f32(x) for x in (b1, 1.0 - b1, b2, 1.0 - b2, lr / (1.0 - b1 ** t), np.sqrt(1.0 - b2 ** t), eps))


def adam(tot, gacc, m, v, theta, active, skipped, mask, accumulate, scalars, lo=None, hi=None):
    """npa_lon_adam -> (tot, gacc, m, v, theta, skipped) after the call"""
    b1, omb1, b2, omb2, step_size, bc2_sqrt, eps = scalars
    lo = np.full(8, -np.inf, dtype=f32) if lo is None else np.asarray(lo, dtype=f32)
    hi = np.full(8, np.inf, dtype=f32) if hi is None else np.asarray(hi, dtype=f32)
    tot, gacc = np.array(tot, dtype=f64), np.array(gacc, dtype=f32)
    m, v, theta = np.array(m, dtype=f32), np.array(v, dtype=f32), np.array(theta, dtype=f32)
    with np.errstate(all="ignore"):
        g32 = tot[:, :7].astype(f32)
        gacc[:, :7] = (gacc[:, :7] + g32) if accumulate else g32
        tot[:, :7] = 0.0
        cols = [c for c in range(7) if (mask >> c) & 1]
        finite = np.isfinite(gacc[:, cols]).all(axis=1) if cols else np.ones(len(theta), dtype=bool)
        on = np.asarray(active) != 0
        step = on & finite
        skipped = (np.asarray(skipped) + (on & ~finite)).astype(np.int32)
        for c in cols:
            g = gacc[:, c]
            m1 = b1 * m[:, c] + omb1 * g
            v1 = b2 * v[:, c] + (omb2 * g) * g
            denom = np.sqrt(v1) / bc2_sqrt + eps
            th = theta[:, c] - step_size * (m1 / denom)
            th = np.minimum(np.maximum(th, lo[c]), hi[c])
            m[:, c], v[:, c], theta[:, c] = np.where(step, m1, m[:, c]), np.where(step, v1, v[:, c]), np.where(step, th, theta[:, c])
    for a in (m, v, theta, gacc):
        assert a.dtype == f32
    return tot, gacc, m, v, theta, skipped


# ---------------------------------------------------------------------------------------------------- the decided cases
CYCLES = 8
EPISODES = 3
LANE = 8.0                    # robot b drives along y = LANE * b, heading +x
THETA0 = np.array([[1.0, 1.0, 1.0, 1.0, 15.0, 1.0, 0.1]] * 5 + [[1.0, 1.0, 1.0, 2.0, 10.0, 0.8, 0.1]], dtype=np.float32)
TRAINED = (3, 4, 5)           # p_u, eta, d_max: the example's optimiser


def _pts(xs, y, gear=1):
    return [np.array([[x], [y], [0.0], [float(gear)]]) for x in xs]


def lon_cases(front, cycles=CYCLES):
    """Six robots in lanes, one per decided case (`front` = the largest x of the robot polygon in its own frame):
      0  its polygon starts 0.02 m from a circle: min_distance is below the threshold in cycle 0 -- the collision branch fires
         there, `stop` ends its episode in the same cycle
      1  held still by scripted zeros: its stuck count passes 5 in cycle 5, the stuck branch fires there and ends its episode
      2  a free straight path, driven by the planner: nothing fires
      3  starts 0.05 m from the end of its path: arrives in cycle 0 (no loss: nothing near, not stuck)
      4  scripted at 4 m/s (0.4 m per cycle) towards a polygon 2.2 m ahead of its nose: 0.2 m short of it when cycle 5 plans (above
         the threshold: no loss), 0.2 m inside it after that cycle's step: collided in cycle 5
      5  robot 2's case with another parameter row
    Returns dict(paths, poses [6,3], actions [cycles,6,2] f32 (NaN = the planner's), circles [4,6], polygon [4,2], theta0 [6,7])."""
    y = [LANE * b for b in range(6)]
    step = np.round(np.arange(0, 61) * 0.4, 10)
    paths = [_pts(step, y[0]), _pts(step, y[1]), _pts(step, y[2]), _pts(np.round(np.arange(0, 6) * 0.4, 10), y[3]),
             _pts(step, y[4]), _pts(step, y[5])]
    poses = np.array([[0.0, y[0], 0.0], [0.0, y[1], 0.0], [0.0, y[2] + 0.1, 0.05], [1.95, y[3] + 0.02, 0.0], [0.0, y[4], 0.0],
                      [0.0, y[5] + 0.1, -0.05]])
    a = np.full((cycles, 6, 2), np.nan, dtype=np.float32)
    a[:, 1] = [0.0, 0.0]
    a[:, 4] = [4.0, 0.0]
    r = 0.5
    circles = np.array([[front + 0.02 + r, y[0], r, 0, 0, 0], [3.0, y[1] + 2.4, r, 0, 0, 0], [4.0, y[2] + 2.4, r, 0, 0, 0],
                        [4.0, y[5] + 2.4, r, 0, 0, 0]])
    x0 = front + 2.2
    polygon = np.array([[x0, y[4] - 1.5], [x0 + 1.0, y[4] - 1.5], [x0 + 1.0, y[4] + 1.5], [x0, y[4] + 1.5]])
    return dict(paths=paths, poses=poses, actions=a, circles=circles, polygon=polygon, theta0=THETA0.copy())


def straight_cases(B=6):
    """robots that drive and never stop, arrive, collide or stand still within 16 cycles (training off = the plain loop)"""
    paths = [_pts(np.arange(0, 60) * 0.4, LANE * b) for b in range(B)]
    poses = np.column_stack([np.zeros(B), LANE * np.arange(B) + 0.1, np.linspace(-0.2, 0.2, B)])
    circles = np.array([[4.0, LANE * b + 2.4, 0.5, 0, 0, 0] for b in range(B)] + [[7.0, -3.0, 0.4, -0.5, 0.3, 0]])
    return paths, poses, circles
