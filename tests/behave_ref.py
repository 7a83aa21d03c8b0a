"""The definition of npa_world_behave (include/neupan_amd.h) restated in fp64 numpy, operator for operator, for
tests/test_behave*.py.  The method: van den Berg, Lin, Manocha, "Reciprocal Velocity Obstacles for Real-Time Multi-Agent
Navigation", ICRA 2008 -- the sampled penalty w / tc + |v_pref - v'|.

One world at a time, every candidate against every neighbour: no culling, no chunks.
    circles  (C, 6)  cx, cy, r, vx, vy, 0            segments (S, 6)  ax, ay, bx, by, vx, vy
    rows     (A, 10) gx gy vx vy ox oy R v_max goal_threshold chosen      idx (A, 4) first count wander draws
"""
import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
INF = np.inf


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniform(seed, world, agent, draw, coord):
    z = mix((int(seed) + int(world)) & M64)
    z = mix((z + int(agent)) & M64)
    z = mix((z + int(draw)) & M64)
    z = mix((z + int(coord)) & M64)
    return float(z >> 11) * 2.0 ** -53


def draw_goal(seed, world, agent, draw, lo, hi):
    return np.array([float(lo[k]) + (float(hi[k]) - float(lo[k])) * uniform(seed, world, agent, draw, k) for k in (0, 1)])


def agent_ok(first, count, nC, nS):
    return first >= 0 and count >= 1 and (count == 1 if first < nC else first - nC + count <= nS)


def candidates(v_pref, v_cur, v_max, dirs, n_speed):
    """(n_cand, 2): 0, v_pref, v_cur (scaled to v_max when faster), then the grid"""
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 2)
    sp = np.sqrt(v_cur[0] * v_cur[0] + v_cur[1] * v_cur[1])
    vc = np.array(v_cur, dtype=np.float64)
    if sp > v_max:
        sc = v_max / sp
        vc = np.array([v_cur[0] * sc, v_cur[1] * sc])
    out = [np.zeros(2), np.array(v_pref, dtype=np.float64), vc]
    if len(dirs) and n_speed > 0:
        for j in range(n_speed):
            s = (v_max * float(j + 1)) / float(n_speed)
            for k in range(len(dirs)):
                out.append(np.array([s * dirs[k, 0], s * dirs[k, 1]]))
    return np.array(out)


def disc_tc(cx, cy, c2, ux, uy):
    """arrays over the candidates; +inf: no collision"""
    b = cx * ux + cy * uy
    u2 = ux * ux + uy * uy
    disc = b * b - u2 * c2
    if c2 <= 0.0:
        return np.where(b > 0.0, 0.0, INF)
    hit = (b > 0.0) & (disc >= 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = c2 / (b + np.sqrt(np.where(hit, disc, 0.0)))
    return np.where(hit, t, INF)


def seg_tc(wx, wy, ex, ey, ux, uy):
    wxe = wx * ey - wy * ex
    det = ux * ey - uy * ex
    un = wx * uy - wy * ux
    neg = det < 0.0
    ad, tn, us = np.where(neg, -det, det), np.where(neg, -wxe, wxe), np.where(neg, -un, un)
    valid = (ad > 0.0) & (tn >= 0.0) & (us >= 0.0) & (us <= ad)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = tn / np.where(valid, ad, 1.0) + 0.0
    return np.where(valid, t, INF)


def behave_world(circles, segments, rows, idx, par, robots, prev_robots, robot_radius, seg_limit, dirs, n_speed, dt, world=0,
                 counts=None):
    """One call of npa_world_behave for one world.  par: dict(weight, horizon, robot_share, range_low, range_high, seed);
    robots (R, 3): the robots this world's agents see; prev_robots (R, 3) or None; world: world_base + w; counts: None (the
    arrays' lengths), or (n_circles, n_segments, n_agents) as the count arrays hold them: each is clamped to [0, the array's
    length], and the rows at and beyond it are neither read nor written (they come back as they went in).
    Returns dict(circles, segments, rows, idx: the arrays after the call; chosen (A,) int; costs: list of (n_cand,) arrays;
    tc: list of (n_cand,) arrays; None for rows that are no agents), A the clamped number of agents."""
    C_all = np.array(circles, dtype=np.float64).reshape(-1, 6)
    S_all = np.array(segments, dtype=np.float64).reshape(-1, 6)
    rows_all = np.array(rows, dtype=np.float64).reshape(-1, 10)
    idx_all = np.array(idx, dtype=np.int64).reshape(-1, 4)
    nC, nS, nA = len(C_all), len(S_all), len(rows_all)
    if counts is not None:
        nC, nS, nA = (min(max(int(n), 0), full) for n, full in zip(counts, (nC, nS, nA)))
    C, S, rows, idx = C_all[:nC], S_all[:nS], rows_all[:nA], idx_all[:nA]           # (views: launch 2 writes through them)
    robots = np.zeros((0, 3)) if robots is None else np.asarray(robots, dtype=np.float64).reshape(-1, 3)
    ok = [agent_ok(int(idx[k, 0]), int(idx[k, 1]), nC, nS) for k in range(nA)]
    owned = np.zeros(nC + nS, dtype=bool)
    for k in range(nA):
        if ok[k]:
            owned[idx[k, 0]:idx[k, 0] + idx[k, 1]] = True

    def anchor(f):
        return (C[f, 0:2], C[f, 3:5]) if f < nC else (S[f - nC, 0:2], S[f - nC, 4:6])

    w, hz, al_r = float(par["weight"]), float(par["horizon"]), float(par["robot_share"])
    inv_r = 1.0 / al_r
    nSv = min(seg_limit, nS) if seg_limit >= 0 else nS
    new_rows, new_idx = rows.copy(), idx.copy()
    chosen, costs, tcs = np.full(nA, -1, dtype=np.int64), [None] * nA, [None] * nA
    for a in range(nA):
        if not ok[a]:
            continue
        first, wander, draws = int(idx[a, 0]), int(idx[a, 2]), int(idx[a, 3]) & M32     # (the int32 column holds a uint32)
        anc, vA = anchor(first)
        px, py = anc[0] + rows[a, 4], anc[1] + rows[a, 5]
        RA, vmax, thr = rows[a, 6], rows[a, 7], rows[a, 8]
        vax, vay = float(vA[0]), float(vA[1])
        # ---- step 1
        gx, gy = rows[a, 0], rows[a, 1]
        dx, dy = gx - px, gy - py
        L = np.sqrt(dx * dx + dy * dy)
        arrived = L <= thr
        redraw = arrived and wander != 0
        if redraw:
            gx, gy = draw_goal(par["seed"], world, first, draws, par["range_low"], par["range_high"])
            draws = (draws + 1) & M32
            dx, dy = gx - px, gy - py
            L = np.sqrt(dx * dx + dy * dy)
        if (arrived and not redraw) or not (L > 0.0):
            vp = np.zeros(2)
        else:
            s = min(vmax, L / dt)
            vp = np.array([(dx / L) * s, (dy / L) * s])
        # ---- step 2
        V = candidates(vp, (vax, vay), vmax, dirs, n_speed)
        vx, vy = V[:, 0], V[:, 1]
        tc = np.full(len(V), INF)

        def take(t):
            nonlocal tc
            tc = np.where((t <= hz) & (t < tc), t, tc)

        def disc(ctr, rB, vB, al, inv):
            cx, cy, rho = ctr[0] - px, ctr[1] - py, RA + rB
            apx, apy = (1.0 - al) * vax + al * vB[0], (1.0 - al) * vay + al * vB[1]
            c2 = (cx * cx + cy * cy) - rho * rho
            take(disc_tc(cx, cy, c2, (vx - apx) * inv, (vy - apy) * inv))

        # ---- steps 3 and 4
        for p in range(nC):
            if not owned[p]:
                disc(C[p, 0:2], C[p, 2], C[p, 3:5], 1.0, 1.0)
        for k in range(nA):
            if k != a and ok[k]:
                ancB, vB = anchor(int(idx[k, 0]))
                disc((ancB[0] + rows[k, 4], ancB[1] + rows[k, 5]), rows[k, 6], vB, 0.5, 2.0)
        for r in range(len(robots)):
            if prev_robots is None:
                vB = (0.0, 0.0)
            else:
                vB = ((robots[r, 0] - prev_robots[r][0]) / dt, (robots[r, 1] - prev_robots[r][1]) / dt)
            disc(robots[r, 0:2], robot_radius, vB, al_r, inv_r)
        for p in range(nSv):
            if owned[nC + p]:
                continue
            q = S[p]
            wx, wy, bx, by = q[0] - px, q[1] - py, q[2] - px, q[3] - py
            ex, ey = q[2] - q[0], q[3] - q[1]
            ux, uy = vx - q[4], vy - q[5]
            e2 = ex * ex + ey * ey
            ln = np.sqrt(e2)
            nx, ny = ((ey / ln) * RA, ((-ex) / ln) * RA) if e2 > 0.0 else (0.0, 0.0)
            t = disc_tc(wx, wy, (wx * wx + wy * wy) - RA * RA, ux, uy)
            t = np.minimum(t, disc_tc(bx, by, (bx * bx + by * by) - RA * RA, ux, uy))
            t = np.minimum(t, seg_tc(wx + nx, wy + ny, ex, ey, ux, uy))
            t = np.minimum(t, seg_tc(wx - nx, wy - ny, ex, ey, ux, uy))
            take(t)
        # ---- step 5
        ddx, ddy = vp[0] - vx, vp[1] - vy
        with np.errstate(divide="ignore"):
            cost = w / tc + np.sqrt(ddx * ddx + ddy * ddy)
        best = int(np.argmin(cost)) if np.isfinite(cost).any() else 0          # (argmin: the first minimum, the lowest index)
        chosen[a], costs[a], tcs[a] = best, cost, tc
        new_rows[a, 0:4] = [gx, gy, V[best, 0], V[best, 1]]
        new_rows[a, 9] = float(best)
        new_idx[a, 3] = draws - (1 << 32) if draws >> 31 else draws               # (back into the int32 column)
    # ---- launch 2
    for a in range(nA):
        if ok[a]:
            for p in range(int(idx[a, 0]), int(idx[a, 0] + idx[a, 1])):
                if p < nC:
                    C[p, 3:5] = new_rows[a, 2:4]
                else:
                    S[p - nC, 4:6] = new_rows[a, 2:4]
    rows_all[:nA], idx_all[:nA] = new_rows, new_idx
    return dict(circles=C_all, segments=S_all, rows=rows_all, idx=idx_all, chosen=chosen, costs=costs, tc=tcs)


def decided(costs, rel=1e-12):
    """the restatement's two lowest costs differ by more than `rel` relative (or only one is finite, or none): the choice does
    not hang on a rounding"""
    c = np.sort(np.asarray(costs, dtype=np.float64))
    if len(c) < 2 or not np.isfinite(c[0]):
        return True                                              # all infinite: index 0 by rule
    if not np.isfinite(c[1]):
        return True
    return (c[1] - c[0]) > rel * max(abs(c[1]), abs(c[0]))


def move(circles, segments, dt):
    """npa_world_step's translation of the moving primitives (no bounds)"""
    C, S = np.array(circles, dtype=np.float64), np.array(segments, dtype=np.float64)
    for q in C:
        if q[3] != 0 or q[4] != 0:
            q[0] += q[3] * dt; q[1] += q[4] * dt
    for q in S:
        if q[4] != 0 or q[5] != 0:
            q[0] += q[4] * dt; q[2] += q[4] * dt
            q[1] += q[5] * dt; q[3] += q[5] * dt
    return C, S


def run_case(case, world_base=0):
    """every world of a case of tests/behave_cases.py through behave_world; world w sees robot w when there are as many worlds
    as robots, else all of them.  Returns the list of behave_world's dicts."""
    W, B = len(case["worlds"]), len(case["robots"])
    out = []
    for w, wd in enumerate(case["worlds"]):
        sel = slice(w, w + 1) if (W == B and W > 1) or B == 1 else slice(0, B)
        prev = None if case["prev"] is None else case["prev"][sel]
        out.append(behave_world(wd["circles"], wd["segments"], wd["rows"], wd["idx"], case["par"], case["robots"][sel], prev,
                                case["radius"], case["seg_limit"], case["dirs"], case["n_speed"], case["dt"], world=world_base + w))
    return out


def centres(circles, segments, rows, idx):
    """(A, 2) the agents' centres: anchor + offset"""
    C, S = np.asarray(circles).reshape(-1, 6), np.asarray(segments).reshape(-1, 6)
    out = np.zeros((len(rows), 2))
    for a in range(len(rows)):
        f = int(idx[a][0])
        out[a] = (C[f, 0:2] if f < len(C) else S[f - len(C), 0:2]) + np.asarray(rows)[a, 4:6]
    return out


def simulate(wd, par, cycles, dt, dirs, n_speed, robots=None, world=0):
    """`cycles` times behave_world, then the translation; robots: None, or (cycles + 1, R, 3) poses (prev = the row before; the
    first cycle passes none).  Returns dict(world: the arrays after the last cycle, centres (cycles + 1, A, 2), gap: the smallest
    distance between two agents' discs over all cycles, chosen (cycles, A))."""
    C, S, rows, idx = wd["circles"], wd["segments"], wd["rows"], wd["idx"]
    hist, chosen = [centres(C, S, rows, idx)], []
    R = np.asarray(rows)[:, 6]
    gap = INF
    for cyc in range(cycles):
        rb = None if robots is None else robots[cyc]
        pv = None if robots is None or cyc == 0 else robots[cyc - 1]
        o = behave_world(C, S, rows, idx, par, rb, pv, 0.0 if robots is None else par.get("robot_radius", 0.5), -1, dirs, n_speed, dt,
                         world=world)
        C, S = move(o["circles"], o["segments"], dt)
        rows, idx = o["rows"], o["idx"]
        chosen.append(o["chosen"])
        P = centres(C, S, rows, idx)
        hist.append(P)
        for a in range(len(P)):
            for b in range(a + 1, len(P)):
                gap = min(gap, float(np.hypot(*(P[a] - P[b])) - (R[a] + R[b])))
    return dict(world=dict(circles=C, segments=S, rows=rows, idx=idx), centres=np.array(hist), gap=gap, chosen=np.array(chosen))
