"""npa_lon_reduce and npa_lon_scatter (csrc/lon.hip) restated in numpy, operation for operation.

The reduce kernel keeps eight slot sums per column: slot s adds the members s, s + 8, s + 16, ... of a group in that order, one
float64 addition each, starting from +0.0; then slots 4..7 are added to 0..3, 2..3 to 0..1 and 1 to 0, the lower slot on the left
(include/neupan_amd.h).  numpy's float64 does the same single IEEE operations, so the GPU tests compare with array_equal."""
import numpy as np

f32, f64 = np.float32, np.float64


def slot_sum(x):
    """x [n, C] float64 -> (C,): the kernel's sum over the n rows, in its order"""
    x = np.asarray(x, dtype=f64)
    n, C = x.shape
    a = np.zeros((8, C), dtype=f64)                              # +0.0
    with np.errstate(all="ignore"):
        for i in range((n + 7) // 8):                            # the trips of the wave
            for s in range(8):
                j = i * 8 + s
                a[s] = a[s] + (x[j] if j < n else np.zeros(C, dtype=f64))   # (a slot past the end adds +0.0)
        for half in (4, 2, 1):
            for s in range(half):
                a[s] = a[s] + a[s + half]
    return a[0].copy()


def reduce(group_first, group_members, tot, active, loss, mask, mean, dropped):
    """npa_lon_reduce -> dict(tot, gtot_cols (G, 7), gactive, n_used, dropped, gloss) after the call (gtot's column 7 is not
    written by the kernel and not part of the result); loss may be None (gloss is then all +0.0: the kernel's sum)"""
    first, members = np.asarray(group_first), np.asarray(group_members)
    tot_in = np.asarray(tot, dtype=f64)
    tot_out = tot_in.copy()
    active = np.asarray(active)
    G = len(first) - 1
    cols = [c for c in range(7) if (mask >> c) & 1]
    gtot, gloss = np.zeros((G, 7), dtype=f64), np.zeros(G, dtype=f64)
    n_used, dropped = np.zeros(G, dtype=np.int32), np.array(dropped, dtype=np.int32)
    with np.errstate(all="ignore"):
        for g in range(G):
            mem = members[first[g]:first[g + 1]]
            n = len(mem)
            x = np.zeros((n, 8), dtype=f64)
            used = 0
            for j, b in enumerate(mem):
                on = active[b] != 0
                fin = bool(np.isfinite(tot_in[b, cols].astype(f32)).all()) if cols else True
                use = on and fin
                if use:
                    x[j, :7] = tot_in[b, :7]
                if loss is not None and on:
                    x[j, 7] = f64(f32(loss[b]))
                used += int(use)
                dropped[g] += int(on and not fin)
                tot_out[b, :7] = 0.0
            a = slot_sum(x)
            n_used[g] = used
            gtot[g] = a[:7] / f64(used) if (mean and used > 0) else a[:7]
            gloss[g] = a[7]
    return dict(tot=tot_out, gtot_cols=gtot, gactive=(n_used > 0).astype(np.int32), n_used=n_used, dropped=dropped, gloss=gloss)


def scatter(group_of, group_theta, theta):
    """npa_lon_scatter -> theta after the call"""
    group_of, gt = np.asarray(group_of), np.asarray(group_theta, dtype=f32)
    out = np.array(theta, dtype=f32)
    ok = (group_of >= 0) & (group_of < gt.shape[0])
    out[ok, :7] = gt[group_of[ok], :7]
    return out


# ---------------------------------------------------------------------------------------------------- the group layouts
def layouts():
    """{name: (B, group numbers [B])}: the shapes of the kernel tests.  One member; 1, 5 and 64 members interleaved over the
    robot index; 129 (17 trips and a ragged last one), 0, 8 and 1 members with two robots in no group."""
    one = np.zeros(1, dtype=np.int64)
    b70 = np.full(70, 2, dtype=np.int64)
    b70[33] = 0
    b70[[3, 17, 31, 45, 59]] = 1
    b140 = np.full(140, 0, dtype=np.int64)
    b140[[5, 21, 37, 53, 69, 85, 101, 117]] = 2
    b140[64] = 3
    b140[[0, 139]] = -1
    tabs = {"B1_G1": (1, one), "B70_G3": (70, b70), "B140_G4": (140, b140)}
    assert [int((b70 == g).sum()) for g in range(3)] == [1, 5, 64]
    assert [int((b140 == g).sum()) for g in range(4)] == [129, 0, 8, 1] and int((b140 == -1).sum()) == 2
    return tabs
