"""A numpy float64 restatement of one DUNE training step, written from include/neupan_amd_train.h: the forward pass of
the 2 -> 32 -> 32 -> 32 -> 32 -> 32 -> E network, the four losses, the backward pass by hand (LayerNorm included) and
the Adam step.  It shares no code with neupan_amd.dune_train; tests/test_dune_train_engine.py holds it against float64
torch autograd, and it documents the formulas the kernel implements."""
import numpy as np

KEYS = ("MLP.0.weight", "MLP.0.bias", "MLP.1.weight", "MLP.1.bias", "MLP.3.weight", "MLP.3.bias", "MLP.5.weight", "MLP.5.bias",
        "MLP.6.weight", "MLP.6.bias", "MLP.8.weight", "MLP.8.bias", "MLP.10.weight", "MLP.10.bias", "MLP.11.weight", "MLP.11.bias",
        "MLP.13.weight", "MLP.13.bias")
# the header's offsets up to the last layer; MLP.13.weight at 4512, MLP.13.bias at 4512 + 32 E
OFFSETS = (0, 64, 96, 128, 160, 1184, 1216, 2240, 2272, 2304, 2336, 3360, 3392, 4416, 4448, 4480, 4512)
LN_EPS = 1e-5


def shapes(E):
    return [(32, 2), (32,), (32,), (32,), (32, 32), (32,), (32, 32), (32,), (32,), (32,), (32, 32), (32,), (32, 32), (32,), (32,),
            (32,), (E, 32), (E,)]


def param_count(E):
    return 4512 + 33 * E


def unpack(flat, E):
    """{key: float64 array} from a pack."""
    out, off = {}, 0
    for k, sh in zip(KEYS, shapes(E)):
        n = int(np.prod(sh))
        out[k] = np.asarray(flat[off:off + n], dtype=np.float64).reshape(sh)
        off += n
    assert off == param_count(E) == len(flat)
    return out


def pack(w):
    return np.concatenate([np.asarray(w[k], dtype=np.float64).reshape(-1) for k in KEYS])


def _block_fwd(x, W, b, g, be, W2, b2):
    z = x @ W.T + b
    mean = z.mean(axis=1, keepdims=True)
    var = ((z - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    xh = (z - mean) * rstd
    t = np.tanh(xh * g + be)
    r = np.maximum(t @ W2.T + b2, 0.0)
    return r, (x, xh, rstd, t, r)


def _block_bwd(dr, saved, W, g, W2):
    """dr: gradient at the block's ReLU output.  Returns dx and the gradients of W, b, g, be, W2, b2."""
    x, xh, rstd, t, r = saved
    dz2 = dr * (r > 0)
    dW2, db2 = dz2.T @ t, dz2.sum(axis=0)
    da = (dz2 @ W2) * (1.0 - t * t)
    dg, dbe = (da * xh).sum(axis=0), da.sum(axis=0)
    dxh = da * g
    dz = rstd * (dxh - dxh.mean(axis=1, keepdims=True) - xh * (dxh * xh).mean(axis=1, keepdims=True))
    return dz @ W, (dz.T @ x, dz.sum(axis=0), dg, dbe, dW2, db2)


def losses_and_grad(flat, G, h, points, mu_l, dist_l, cs, want_grad=True):
    """The four losses of one batch and the gradient of their sum with respect to the pack.  G [E,2], h [E], points [b,2],
    mu_l [b,E], dist_l [b], cs = (cos, sin) of the batch's rotation."""
    G, h = np.asarray(G, np.float64), np.asarray(h, np.float64).reshape(-1)
    p, mu_l, dist_l = np.asarray(points, np.float64), np.asarray(mu_l, np.float64), np.asarray(dist_l, np.float64)
    E, b = G.shape[0], p.shape[0]
    w = unpack(flat, E)
    x, saved = p, []
    for i in (0, 5, 10):
        x, sv = _block_fwd(x, w[f"MLP.{i}.weight"], w[f"MLP.{i}.bias"], w[f"MLP.{i + 1}.weight"], w[f"MLP.{i + 1}.bias"],
                           w[f"MLP.{i + 3}.weight"], w[f"MLP.{i + 3}.bias"])
        saved.append(sv)
    mu = x
    gp = p @ G.T - h
    dist = (mu * gp).sum(axis=1)
    c, s = cs
    M = -(np.array([[c, -s], [s, c]], np.float64) @ G.T)                 # [2,E]
    fa, fa_l = mu @ M.T, mu_l @ M.T
    fb, fb_l = (fa * p).sum(axis=1) + mu @ h, (fa_l * p).sum(axis=1) + mu_l @ h
    losses = np.array([((mu - mu_l) ** 2).sum() / (b * E), ((dist - dist_l) ** 2).sum() / b, ((fa - fa_l) ** 2).sum() / (2 * b),
                       ((fb - fb_l) ** 2).sum() / b])
    if not want_grad:
        return losses, None
    dmu = (2.0 / (b * E)) * (mu - mu_l) + (2.0 / b) * (dist - dist_l)[:, None] * gp + (1.0 / b) * (fa - fa_l) @ M \
        + (2.0 / b) * (fb - fb_l)[:, None] * (p @ M + h)
    grads = {}
    d = dmu
    for i, sv in zip((10, 5, 0), saved[::-1]):
        d, (dW, db, dg, dbe, dW2, db2) = _block_bwd(d, sv, w[f"MLP.{i}.weight"], w[f"MLP.{i + 1}.weight"], w[f"MLP.{i + 3}.weight"])
        grads.update({f"MLP.{i}.weight": dW, f"MLP.{i}.bias": db, f"MLP.{i + 1}.weight": dg, f"MLP.{i + 1}.bias": dbe,
                      f"MLP.{i + 3}.weight": dW2, f"MLP.{i + 3}.bias": db2})
    return losses, pack(grads)


def adam_step(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam's update; t = the number of this step (1 for the first).  Returns p, m, v."""
    g = g + weight_decay * p
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - (lr / (1.0 - beta1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps)
    return p, m, v
