"""The fused DUNE training step, the parts that need no GPU: the float64 restatement (tests/dune_train_ref.py) against
float64 torch autograd of `dune_losses`; the ABI of libneupan_amd_train.so (include/neupan_amd_train.h), its refusals and
its kernel's resources; the parameter pack; the `engine=` argument of DuneTrain.start.  (The library's build contract:
tests/test_build.py.)"""
import ctypes as C
import inspect
import os
import re
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import dune_train_ref as ref  # noqa: E402


def _golden():
    return np.load(os.path.join(HERE, "golden", "dune_train_losses.npz"))


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import _lib_train
    return _lib_train.load()


def _header():
    txt = open(os.path.join(ROOT, "include", "neupan_amd_train.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_restatement_matches_float64_autograd():
    """Losses and every parameter gradient of the hand-written backward pass against torch autograd, both float64, on the
    golden weights and points, one full and one short batch: <= 1e-12 of each tensor's largest gradient."""
    from neupan_amd.dune_train import PACK_KEYS, ObsPointNet, dune_losses
    z = _golden()
    net = ObsPointNet(2, 4).double()
    net.load_state_dict({k[2:]: torch.tensor(z[k]).double() for k in z.files if k.startswith("w/")})
    flat = ref.pack({k: z["w/" + k] for k in ref.KEYS})
    assert tuple(PACK_KEYS) == ref.KEYS
    G, h = torch.tensor(z["G"]).double(), torch.tensor(z["h"]).double()
    for lo, hi, theta in ((0, 256, 0.7), (512, 600, 4.1)):
        P, MU, D = (torch.tensor(z[k][lo:hi]).double() for k in ("points", "mu", "dist"))
        net.zero_grad()
        ls = dune_losses(net, G, h, P, MU, D, theta)
        sum(ls).backward()
        got_l, got_g = ref.losses_and_grad(flat, z["G"], z["h"], z["points"][lo:hi], z["mu"][lo:hi], z["dist"][lo:hi],
                                           (float(np.cos(theta)), float(np.sin(theta))))
        want_l = np.array([float(x.detach()) for x in ls])
        assert np.all(np.abs(got_l - want_l) <= 1e-12 * np.abs(want_l)), (got_l, want_l)
        gg = ref.unpack(got_g, 4)
        for k, p in net.named_parameters():
            want = p.grad.numpy()
            err = np.abs(gg[k] - want).max() / np.abs(want).max()
            assert err <= 1e-12, (k, err)


def test_restatement_adam_matches_torch():
    rng = np.random.default_rng(3)
    p0, m, v = rng.normal(size=50), np.zeros(50), np.zeros(50)
    tp = torch.nn.Parameter(torch.tensor(p0))
    opt = torch.optim.Adam([tp], lr=1e-3, weight_decay=1e-4)
    p = p0.copy()
    for t in range(1, 6):
        g = rng.normal(size=50)
        tp.grad = torch.tensor(g)
        opt.step()
        p, m, v = ref.adam_step(p, g, m, v, t, 1e-3, weight_decay=1e-4)
        assert np.abs(p - tp.detach().numpy()).max() <= 1e-14


def test_prototypes_have_the_argument_counts_of_the_header():
    """(that the names are the header's, bound and exported: tests/test_build.py)"""
    from neupan_amd import _lib_train
    hdr = _header()
    for n in _lib_train.SYMBOLS:
        args = re.search(rf"\b{n}\s*\(([^)]*)\)", hdr).group(1).strip()
        count = 0 if args == "void" else args.count(",") + 1
        assert count == len(_lib_train.SYMBOLS[n][1]), (n, count)


def test_param_count(lib):
    for E in range(3, 9):
        assert lib.npa_dune_train_param_count(E) == 4512 + 33 * E == ref.param_count(E)
    for E in (-1, 0, 2, 9, 64):
        assert lib.npa_dune_train_param_count(E) < 0
        assert b"npa_dune_train_param_count" in lib.npa_dune_train_last_error()


def test_refusals_before_any_device(lib):
    """Every argument the header forbids: NPA_E_ARG and a message that names the export; the pointers are never dereferenced."""
    P = C.c_void_p(0x1000)
    names = ["G", "h", "points", "mu", "dist", "rot", "params", "adam_m", "adam_v", "step_count", "losses", "grad_out"]

    def call(runs=1, E=4, n=600, first_row=0, batch=256, steps=3, train=1, null=()):
        ptr = {k: (None if k in null else P) for k in names}
        return lib.npa_dune_train_steps(runs, E, ptr["G"], ptr["h"], n, ptr["points"], ptr["mu"], ptr["dist"], first_row, batch, steps,
                                        ptr["rot"], 1e-4, 0.9, 0.999, 1e-8, 1e-4, train, ptr["params"], ptr["adam_m"], ptr["adam_v"],
                                        ptr["step_count"], ptr["losses"], ptr["grad_out"], None)

    def refused(rc):
        assert rc == -1, rc
        assert b"npa_dune_train_steps" in lib.npa_dune_train_last_error()

    for kw in (dict(runs=0), dict(runs=-2), dict(batch=0), dict(steps=0), dict(E=2), dict(E=9), dict(n=0), dict(first_row=-1),
               dict(steps=4),                                   # rows 768.. of 600: an empty step
               dict(first_row=600, steps=1), dict(first_row=89, steps=3)):
        refused(call(**kw))
    for k in ("G", "h", "points", "mu", "dist", "rot", "params", "losses"):
        refused(call(null=(k,)))
        refused(call(null=(k,), train=0))
    for k in ("adam_m", "adam_v", "step_count"):
        refused(call(null=(k,)))                                # required when training ..


def test_pack_round_trip_and_offsets():
    from neupan_amd.dune_train import PACK_KEYS, ObsPointNet, pack_layout, pack_params, unpack_params
    z = _golden()
    for E in (3, 4, 8):
        torch.manual_seed(E)
        net = ObsPointNet(2, E)
        assert list(net.state_dict().keys()) == list(PACK_KEYS)
        if E == 4:
            assert sorted(PACK_KEYS) == sorted(k[2:] for k in z.files if k.startswith("w/"))     # the reference's keys
        flat = pack_params(net)
        lay, P = pack_layout(E)
        assert flat.dtype == torch.float32 and flat.shape == (P,) and P == ref.param_count(E)
        assert [lay[k][0] for k in PACK_KEYS[:17]] == list(ref.OFFSETS) and lay["MLP.13.bias"][0] == 4512 + 32 * E
        for k, (off, sh) in lay.items():
            assert torch.equal(flat[off:off + int(np.prod(sh))].reshape(sh), net.state_dict()[k])
        other = ObsPointNet(2, E)
        unpack_params(flat, other)
        assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), other.state_dict().values()))
        assert torch.equal(pack_params(other), flat)
    with pytest.raises(ValueError):
        unpack_params(torch.zeros(10), ObsPointNet(2, 4))


def test_engine_argument():
    from neupan_amd.dune_train import DuneTrain, ObsPointNet
    z = _golden()
    assert inspect.signature(DuneTrain.start).parameters["engine"].default == "torch"
    tr = DuneTrain(None, z["G"], z["h"], tempfile.mkdtemp(), device="cpu")
    with pytest.raises(ValueError, match="engine"):
        tr.start(data_size=100, epoch=0, engine="nope")
    foreign = torch.nn.Sequential(torch.nn.Linear(2, 4), torch.nn.ReLU())
    with pytest.raises(ValueError, match="ObsPointNet"):
        DuneTrain(foreign, z["G"], z["h"], tempfile.mkdtemp(), device="cpu").start(data_size=100, epoch=0, engine="hip")
    with pytest.raises(ValueError, match="ObsPointNet"):        # the right class, the wrong width
        DuneTrain(ObsPointNet(2, 5), z["G"], z["h"], tempfile.mkdtemp(), device="cpu").start(data_size=100, epoch=0, engine="hip")
    assert not os.path.exists(os.path.join(tr.checkpoint_path, "results.txt"))      # refused before anything is written


def test_training_kernel_has_no_scratch_and_no_spills(lib):
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import kernel_resources as kr
    from neupan_amd import build as b
    if not kr.tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    res = {n: r for n, r in kr.kernel_resources(lib=b.TRAIN_LIB).items() if "dune_train_kernel" in n}
    assert len(res) == 1, sorted(res)                           # one instantiation: E is a run-time value
    (r,) = res.values()
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    # (vgpr_count of the metadata is the unified total, accumulation registers included: one wave per SIMD has 512)
    assert r["agpr"] <= r["vgpr"] <= 512 and r["lds"] <= 160 * 1024, r
