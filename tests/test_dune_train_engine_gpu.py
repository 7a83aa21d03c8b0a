"""The fused DUNE training step on the device (include/neupan_amd_train.h): losses against the reference's own values,
gradients and a 20-step trajectory against float64 autograd with the project's fp32 torch path as the yardstick, Adam
against torch.optim.Adam, the bitwise properties (split launches, repeats, runs side by side, a short last batch) and
the engine end to end.  Every output array is followed by a poisoned guard that must come back untouched."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, POISON = 512, -777.0
LR, WD = 1e-3, 1e-4


def _golden():
    return np.load(os.path.join(HERE, "golden", "dune_train_losses.npz"))


def guarded(src=None, shape=None, dtype=torch.float32):
    """A device tensor (a copy of `src`, or zeros of `shape`) whose storage continues with GUARD poisoned elements."""
    shape = tuple(src.shape) if src is not None else tuple(shape)
    n = int(np.prod(shape))
    full = torch.full((n + GUARD,), POISON, dtype=dtype, device=DEV)
    view = full[:n].view(shape)
    if src is not None:
        view.copy_(src)
    else:
        view.zero_()
    view._full = full
    return view


def assert_guards(*tensors):
    for t in tensors:
        assert bool((t._full[t.numel():] == POISON).all()), "a guard region was written"


def polygon(E):
    """A convex E-gon around the origin as consecutive counter-clockwise half-planes G x <= h (E = 4: the golden robot)."""
    if E == 4:
        z = _golden()
        return z["G"].astype(np.float32), z["h"].reshape(-1).astype(np.float32)
    a = 2 * np.pi * (np.arange(E) + 0.25) / E - np.pi / 2
    G = np.stack([np.cos(a), np.sin(a)], axis=1) * (1.0 + 0.2 * np.arange(E))[:, None]
    return G.astype(np.float32), (0.8 + 0.1 * np.arange(E)).astype(np.float32)


_CASES = {}


def case(E, n=600):
    """Robot, network, points and labels for edge count E, computed once: a seeded network with its LayerNorm weights and
    biases moved off 1 / 0 and its last bias lowered so that some rows end in an all-zero ReLU; points in +-25 plus (0, 0)
    and the four corners at +-50; labels from the HIP labeller."""
    if (E, n) in _CASES:
        return _CASES[(E, n)]
    from neupan_amd.dune_labels import dune_labels
    from neupan_amd.dune_train import ObsPointNet, pack_params
    G, h = polygon(E)
    rng = np.random.default_rng(100 + E)
    pts = rng.uniform(-25, 25, size=(n, 2))
    pts[:5] = [[0, 0], [50, 50], [-50, 50], [50, -50], [-50, -50]]
    mu, dist = dune_labels(G.astype(np.float64), h.astype(np.float64), pts, torch.device(DEV))
    torch.manual_seed(E)
    net = ObsPointNet(2, E)
    with torch.no_grad():
        for k in (1, 6, 11):
            net.MLP[k].weight.add_(0.2 * torch.randn(32))
            net.MLP[k].bias.add_(0.2 * torch.randn(32))
        x = torch.tensor(pts, dtype=torch.float32)
        net.MLP[13].bias.sub_(torch.quantile(net.MLP[:14](x).max(dim=1).values, 0.3))      # ~30 % of the rows end all-zero
        out = net(x)
    dead = (out == 0).all(dim=1)
    assert 0 < int(dead.sum()) < n, "the case needs rows with an all-zero last ReLU, and rows without"
    c = dict(E=E, n=n, G=G, h=h, net=net, flat=pack_params(net), points=torch.tensor(pts, dtype=torch.float32), mu=mu.float().cpu(),
             dist=dist.float().cpu())
    _CASES[(E, n)] = c
    return c


def device_data(cases):
    """The stacked device inputs of one or several cases (runs)."""
    st = lambda k: torch.stack([torch.as_tensor(c[k]) for c in cases]).to(DEV).contiguous()
    return dict(G=st("G"), h=st("h"), points=st("points"), mu=st("mu"), dist=st("dist"))


def rotations(steps, seed=5):
    th = np.random.default_rng(seed).uniform(0, 2 * np.pi, size=steps)
    return th, torch.tensor(np.stack([np.cos(th), np.sin(th)], axis=1).astype(np.float32), device=DEV)


def launch(d, params, m, v, t, first_row, batch, rot, train=True, grad=None, lr=LR):
    from neupan_amd.dune_train import train_steps
    losses = guarded(shape=(params.shape[0], rot.shape[0], 4))
    train_steps(d["G"], d["h"], d["points"], d["mu"], d["dist"], first_row, batch, rot, params, m, v, t, lr=lr, weight_decay=WD,
                train=train, grad_out=grad, losses=losses)
    torch.cuda.synchronize()
    assert_guards(losses, params, *(x for x in (m, v, t, grad) if x is not None))
    return losses


def fresh_state(cases):
    params = guarded(torch.stack([c["flat"] for c in cases]))
    return params, guarded(shape=params.shape), guarded(shape=params.shape), guarded(shape=(len(cases),), dtype=torch.int32)


def autograd(c, lo, hi, theta, dtype, device):
    """Losses and the packed gradient of their sum by torch autograd of the project's dune_losses, in `dtype` on `device`."""
    import copy
    from neupan_amd.dune_train import PACK_KEYS, dune_losses
    net = copy.deepcopy(c["net"]).to(dtype).to(device)
    cast = lambda x: torch.as_tensor(x).to(dtype).to(device)
    ls = dune_losses(net, cast(c["G"]), cast(c["h"]).reshape(-1, 1), cast(c["points"][lo:hi]), cast(c["mu"][lo:hi]),
                     cast(c["dist"][lo:hi]), theta)
    sum(ls).backward()
    g = dict(net.named_parameters())
    return (np.array([float(x.detach()) for x in ls]), torch.cat([g[k].grad.reshape(-1) for k in PACK_KEYS]).double().cpu().numpy())


def test_losses_match_the_reference_values():
    """train = 0 on the golden file (three batches: 256, 256, 88 rows), the epoch mean against the reference's own values
    at the tolerance of the torch engine's CPU test; nothing but `losses` is written."""
    from neupan_amd.dune_train import ObsPointNet, pack_params, train_steps
    z = _golden()
    net = ObsPointNet(2, 4)
    net.load_state_dict({k[2:]: torch.tensor(z[k]) for k in z.files if k.startswith("w/")})
    c = dict(G=z["G"], h=z["h"].reshape(-1), points=z["points"].astype(np.float32), mu=z["mu"].astype(np.float32),
             dist=z["dist"].astype(np.float32), flat=pack_params(net))
    d = device_data([c])
    np.random.seed(11)                                   # one rotation angle per batch, same draw order
    th = np.array([np.random.uniform(0, 2 * np.pi) for _ in range(3)])
    rot = torch.tensor(np.stack([np.cos(th), np.sin(th)], axis=1).astype(np.float32), device=DEV)
    params, m, v, t = fresh_state([c])
    m.fill_(0.5); v.fill_(0.25); t.fill_(7)
    before = [x.clone() for x in (params, m, v, t)]
    losses = launch(d, params, m, v, t, 0, 256, rot, train=False)
    assert all(torch.equal(a, b) for a, b in zip(before, (params, m, v, t)))
    got = losses[0].double().cpu().numpy().mean(axis=0)
    print("losses", got, "reference", z["losses"], "relative", np.abs(got / z["losses"] - 1))
    assert np.allclose(got, z["losses"], rtol=2e-5, atol=0), (got, z["losses"])
    nul = guarded(shape=(1, 3, 4))                       # the state arrays may be NULL when nothing is trained
    train_steps(d["G"], d["h"], d["points"], d["mu"], d["dist"], 0, 256, rot, params, train=False, losses=nul)
    torch.cuda.synchronize()
    assert torch.equal(nul, losses) and torch.equal(params, before[0])
    assert_guards(nul, params)


BATCHES = (1, 31, 32, 33, 64, 255, 256, 257)


@pytest.mark.parametrize("E", [3, 4, 5, 8])
def test_gradients_against_float64_autograd(E):
    """grad_out of one step against float64 autograd, per parameter tensor in max-norm relative to the tensor's largest
    float64 gradient.  The bar is measured here: 4 x the error of the project's fp32 torch path against the same float64
    values, pooled (the largest) over the batches -- the factor covers another order of the sums over up to 257 rows and
    the device tanh / reciprocal square root.

    Measured on MI355X (worst tensor, hip / torch-fp32 pooled error): see DESIGN.md section 3.5."""
    from neupan_amd.dune_train import pack_layout
    c = case(E)
    d = device_data([c])
    lay, P = pack_layout(E)
    err_hip, err_t32 = {k: [] for k in lay}, {k: [] for k in lay}
    for i, b in enumerate(BATCHES):
        lo = 5 * i                                       # (rows 0 .. 4 -- the origin and the corners -- are in some batches)
        th, rot = rotations(1, seed=b)
        params, m, v, t = fresh_state([c])
        grad = guarded(shape=(1, P))
        losses = launch(d, params, m, v, t, lo, b, rot, grad=grad)
        assert int(t[0]) == 1
        l64, g64 = autograd(c, lo, lo + b, th[0], torch.float64, "cpu")
        l32, g32 = autograd(c, lo, lo + b, th[0], torch.float32, DEV)
        assert np.allclose(losses[0, 0].double().cpu().numpy(), l64, rtol=2e-5, atol=0)
        gh = grad[0].double().cpu().numpy()
        for k, (off, sh) in lay.items():
            s = slice(off, off + int(np.prod(sh)))
            ref = np.abs(g64[s]).max()
            if ref == 0.0:
                assert not gh[s].any(), (k, b)
                continue
            err_hip[k].append(np.abs(gh[s] - g64[s]).max() / ref)
            err_t32[k].append(np.abs(g32[s] - g64[s]).max() / ref)
    worst = 0.0
    for k in lay:
        bar = 4 * max(err_t32[k])
        print(f"E={E} {k:14s} hip {max(err_hip[k]):.3e}  torch-fp32 {max(err_t32[k]):.3e}  ratio {max(err_hip[k]) / max(err_t32[k]):.2f}")
        worst = max(worst, max(err_hip[k]) / max(err_t32[k]))
    print(f"E={E} worst ratio hip / torch-fp32 over the tensors: {worst:.2f}")
    for k in lay:
        assert max(err_hip[k]) <= 4 * max(err_t32[k]), (k, max(err_hip[k]), max(err_t32[k]))


def test_adam_against_torch_optimiser():
    """Eight steps; after each, the kernel's grad_out is fed to torch.optim.Adam(lr, weight_decay=1e-4) on a copy of the
    parameters.  Per step taken the two may differ by one rounding of the result and eight of the update:
    eps32 * (|p| / 2 + 8 lr |m^| / (sqrt(v^) + eps)) (the reasoning of test_lon_gpu.py::test_adam_against_torch_optimiser,
    restated for parameters that start at zero, where an ulp of p is no yardstick).

    Measured on the MI355X: no parameter differs from torch's in any of the eight steps (the kernel reproduces the
    roundings of torch's foreach kernels)."""
    c = case(5)
    d = device_data([c])
    P = c["flat"].numel()
    params, m, v, t = fresh_state([c])
    grad = guarded(shape=(1, P))
    tp = torch.nn.Parameter(c["flat"].clone().to(DEV))
    opt = torch.optim.Adam([tp], lr=LR, weight_decay=WD)
    eps32, worst = float(np.finfo(np.float32).eps), 0.0
    _, rot = rotations(8)
    for k in range(8):
        launch(d, params, m, v, t, 64 * k, 64, rot[k:k + 1].contiguous(), grad=grad)
        tp.grad = grad[0].clone()
        opt.step()
        st = opt.state[tp]
        mhat = st["exp_avg"].double() / (1 - 0.9 ** (k + 1))
        vhat = st["exp_avg_sq"].double() / (1 - 0.999 ** (k + 1))
        bound = (k + 1) * eps32 * (tp.detach().double().abs() / 2 + 8 * LR * mhat.abs() / (vhat.sqrt() + 1e-8))
        diff = (params[0].double() - tp.detach().double()).abs()
        ratio = float((diff / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
        worst = max(worst, ratio)
        print(f"Adam step {k + 1}: {int((diff > 0).sum())} of {P} parameters differ, worst |difference| / bound = {ratio:.3f}")
        assert bool((diff <= bound).all()), (k, ratio)
    assert int(t[0]) == 8
    print(f"Adam: worst |p_hip - p_torch| / bound over 8 steps = {worst:.3f}")


def _run(cases, n_rows, batch, split, rot, lr=LR):
    """`sum(split)` steps as len(split) launches; returns the bits of everything the launches wrote."""
    d = device_data(cases)
    for k in ("points", "mu", "dist"):
        d[k] = d[k][:, :n_rows].contiguous()
    params, m, v, t = fresh_state(cases)
    grad = guarded(shape=params.shape)
    losses, s = [], 0
    for k in split:
        losses.append(launch(d, params, m, v, t, s * batch, batch, rot[s:s + k].contiguous(), grad=grad, lr=lr).clone())
        s += k
    return [x.clone() for x in (params, m, v, t, grad)] + [torch.cat(losses, dim=1)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_bitwise_properties():
    """Five steps in one launch = five launches of one = 2 + 3; a repeat; three runs side by side = each alone; a short last
    batch (300 rows: 4 x 64 + 44, and 2 x 128 + 44)."""
    cs = [case(4), dict(case(4)), dict(case(4))]
    for i in (1, 2):                                     # two more robots and networks of the same E
        cs[i]["h"] = cs[0]["h"] * (1.0 + 0.25 * i)
        cs[i]["flat"] = cs[0]["flat"] * (1.0 - 0.1 * i)
        cs[i]["points"] = cs[0]["points"].flip(0).contiguous() if i == 2 else cs[0]["points"]
    _, rot = rotations(5)
    one = _run(cs[:1], 300, 64, [5], rot)
    assert int(one[3][0]) == 5 and not torch.equal(one[0][0], cs[0]["flat"].to(DEV))
    assert _same(one, _run(cs[:1], 300, 64, [5], rot))
    assert _same(one, _run(cs[:1], 300, 64, [1, 1, 1, 1, 1], rot))
    assert _same(one, _run(cs[:1], 300, 64, [2, 3], rot))
    short = _run(cs[:1], 300, 128, [3], rot[:3])
    assert _same(short, _run(cs[:1], 300, 128, [1, 2], rot[:3]))
    three = _run(cs, 300, 64, [5], rot)
    for r in range(3):
        alone = _run(cs[r:r + 1], 300, 64, [5], rot)
        assert all(torch.equal(x[r], y[0]) for x, y in zip(three, alone)), r
    assert not torch.equal(three[0][0], three[0][1])


def test_trajectory_against_float64():
    """20 steps from the same weights and angles: the hip engine and the fp32 torch path (autograd + torch.optim.Adam on the
    device), each against a float64 torch run; the largest parameter error of the hip engine is at most 4 x the torch
    path's (margin as in the gradient test).  Measured values: DESIGN.md section 3.5."""
    import copy
    from neupan_amd.dune_train import dune_losses, pack_params
    c = case(4)
    steps, batch = 20, 30
    th, rot = rotations(steps, seed=9)
    hip = _run([c], c["n"], batch, [steps], rot)[0][0].double().cpu().numpy()

    def torch_run(dtype, device):
        net = copy.deepcopy(c["net"]).to(dtype).to(device)
        cast = lambda x: torch.as_tensor(x).to(dtype).to(device)
        G, h, P, MU, D = cast(c["G"]), cast(c["h"]).reshape(-1, 1), cast(c["points"]), cast(c["mu"]), cast(c["dist"])
        opt = torch.optim.Adam(net.parameters(), lr=LR, weight_decay=WD)
        for s in range(steps):
            opt.zero_grad()
            sl = slice(s * batch, (s + 1) * batch)
            sum(dune_losses(net, G, h, P[sl], MU[sl], D[sl], th[s])).backward()
            opt.step()
        return pack_params(net.double()).cpu().numpy()

    p64, p32 = torch_run(torch.float64, "cpu"), torch_run(torch.float32, DEV)
    e_hip, e_t32 = np.abs(hip - p64).max(), np.abs(p32 - p64).max()
    moved = np.abs(p64 - c["flat"].double().numpy()).max()
    print(f"trajectory, 20 steps: hip {e_hip:.3e}  torch-fp32 {e_t32:.3e}  ratio {e_hip / e_t32:.2f}  (parameters moved by {moved:.3e})")
    assert moved > 10 * LR
    assert e_hip <= 4 * e_t32, (e_hip, e_t32)


def test_engine_end_to_end_and_train_many(tmp_path):
    """DuneTrain.start(engine="hip") with the arguments of test_dune_train.py::test_short_training_run_on_hip_labels, and
    train_many with two robots: each gets the bits of that robot trained alone under the same seed."""
    from gpu_helpers import make_gpu_pan
    from helpers import CONFIGS, make_oracle
    from neupan_amd.dune_train import DuneTrain, train_many
    orc = make_oracle(CONFIGS["diff_1k_T10_K10"])
    G, h = np.asarray(orc.G), np.asarray(orc.h)
    kw = dict(data_size=8000, data_range=[-25, -25, 25, 25], batch_size=256, epoch=40, valid_freq=10, save_freq=40, lr=5e-3,
              decay_freq=1500)
    robots = [(G, h), (G, h * 0.75)]
    alone = []
    for i, (g, hh) in enumerate(robots):
        d = str(tmp_path / f"alone{i}")
        torch.manual_seed(0); np.random.seed(0)
        tr = DuneTrain(None, g, hh, d)
        full = tr.start(engine="hip", **kw)
        assert full.endswith("model_40.pth") and os.path.exists(full)
        assert tr.loss_list[-1] < 0.9 * tr.loss_list[0] and len(tr.loss_list) == 41
        txt = open(os.path.join(d, "results.txt")).read()
        assert "Validate Mu Loss" in txt and "data_size: 8000" in txt and txt.count("Epoch ") == 5
        alone.append((torch.load(full), tr))
    sd, tr = alone[0]
    assert all(torch.equal(v, tr.model.state_dict()[k].cpu()) for k, v in sd.items())      # the model holds what was saved
    pan = make_gpu_pan(CONFIGS["corridor_diff_small"], checkpoint=os.path.join(str(tmp_path / "alone0"), "model_40.pth"), iter_num=1)
    assert pan.E == 4
    dirs = [str(tmp_path / f"many{i}") for i in range(2)]
    trainers, fulls = train_many([r[0] for r in robots], [r[1] for r in robots], dirs, seeds=0, **kw)
    for i in range(2):
        got = torch.load(fulls[i])
        assert list(got.keys()) == list(alone[i][0].keys())
        assert all(torch.equal(got[k], alone[i][0][k]) for k in got), i
        assert trainers[i].loss_list == alone[i][1].loss_list
    assert not torch.equal(alone[0][0]["MLP.13.weight"], alone[1][0]["MLP.13.weight"])
