"""DUNE training on the GPU: `DUNETrain` of the reference (neupan/blocks/dune_train.py:60-343) with the
per-point ECOS solves of its data-set generation (:109-140, "1-2 h on CPU" for 100 k points) replaced by
the closed-form HIP labeller (csrc/dune_labels.hip, neupan_amd/dune_labels.py).

Everything else follows the reference: the ObsPointNet architecture and state_dict keys
(obs_point_net.py:31-46), Adam(lr=1e-4, weight_decay=1e-4) (:71), the 80/20 split (:191-193), the four
loss terms mu / distance / fa / fb with one random rotation per batch (:302-366), the learning-rate decay,
the `model_<epoch>.pth` checkpoints and the `results.txt` log (:180-300).  The optimisation itself is
PyTorch autograd by default (engine="torch"), as it is in the reference; tensors live on the GPU and
batches are slices (the reference's DataLoader does not shuffle either).  engine="hip" runs every epoch
as one launch of the fused training kernel (csrc/dune_train.hip, include/neupan_amd_train.h) instead,
and `train_many` trains several robots side by side with it.
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch

from .dune_labels import dune_labels


class ObsPointNet(torch.nn.Module):
    """obs_point_net.py:25-49 (same layer order, hence the same `MLP.<k>.*` state_dict keys)."""

    def __init__(self, input_dim=2, output_dim=4):
        super().__init__()
        L, H = torch.nn, 32
        self.MLP = L.Sequential(L.Linear(input_dim, H), L.LayerNorm(H), L.Tanh(), L.Linear(H, H), L.ReLU(),
                                L.Linear(H, H), L.LayerNorm(H), L.Tanh(), L.Linear(H, H), L.ReLU(),
                                L.Linear(H, H), L.LayerNorm(H), L.Tanh(), L.Linear(H, output_dim), L.ReLU())

    def forward(self, x):
        return self.MLP(x)


def dune_losses(model, G, h, points, label_mu, label_distance, theta):
    """The four loss terms of dune_train.py:302-366 for one batch.  points (b,2), label_mu (b,E),
    label_distance (b,), G (E,2), h (E,1); theta: the batch's random rotation angle (:349)."""
    mse = torch.nn.functional.mse_loss
    mu = model(points)                                                   # (b,E)
    dist = (mu * (points @ G.T - h.reshape(1, -1))).sum(dim=1)            # cal_distance :368-378
    c, s = float(np.cos(theta)), float(np.sin(theta))
    R = torch.tensor([[c, -s], [s, c]], dtype=points.dtype, device=points.device)
    M = -(R @ G.T)                                                       # fa = (-R G^T mu)^T  :353-354
    fa, fa_l = mu @ M.T, label_mu @ M.T                                  # (b,2)
    hh = h.reshape(-1)
    fb = (fa * points).sum(dim=1) + mu @ hh                              # :356-357
    fb_l = (fa_l * points).sum(dim=1) + label_mu @ hh
    return mse(mu, label_mu), mse(dist, label_distance), mse(fa, fa_l), mse(fb, fb_l)


class DuneTrain:
    """Constructor and `start` keyword arguments as the reference's DUNETrain (:61, :144-157)."""

    def __init__(self, model, robot_G, robot_h, checkpoint_path, device="cuda"):
        self.device = torch.device(device)
        self.G = torch.as_tensor(np.asarray(robot_G, dtype=np.float32)).to(self.device)
        self.h = torch.as_tensor(np.asarray(robot_h, dtype=np.float32).reshape(-1, 1)).to(self.device)
        self.model = (model if model is not None else ObsPointNet(2, self.G.shape[0])).to(self.device)
        self.checkpoint_path = checkpoint_path
        os.makedirs(checkpoint_path, exist_ok=True)
        self.optimizer = torch.optim.Adam(self.model.parameters(), lr=1e-4, weight_decay=1e-4)
        self.loss_list = []

    def generate_data_set(self, data_size=10000, data_range=(-50, -50, 50, 50)):
        """:109-135 with the labels from the HIP labeller.  Returns float32 device tensors."""
        p = np.random.uniform(low=data_range[:2], high=data_range[2:], size=(data_size, 2))
        mu, dist = dune_labels(self.G.double().cpu().numpy(), self.h.double().cpu().numpy(), p, self.device)
        return torch.from_numpy(p.astype(np.float32)).to(self.device), mu, dist

    def _epoch(self, data, batch_size, validate):
        P, MU, D = data
        tot = np.zeros(4)
        nb = 0
        for i in range(0, P.shape[0], batch_size):
            theta = np.random.uniform(0, 2 * np.pi)
            if not validate:
                self.optimizer.zero_grad()
            with torch.set_grad_enabled(not validate):
                lm, ld, la, lb = dune_losses(self.model, self.G, self.h, P[i:i + batch_size], MU[i:i + batch_size],
                                             D[i:i + batch_size], theta)
                if not validate:
                    (lm + ld + la + lb).backward()
                    self.optimizer.step()
            tot += np.array([lm.item(), ld.item(), la.item(), lb.item()])
            nb += 1
        return tuple(tot / max(nb, 1))

    def _prepare(self, data_size, data_range, batch_size, epoch, valid_freq, save_freq, lr, lr_decay, decay_freq):
        """The head of the log, train_dict.pkl, the learning rate, the data set and its 80/20 split (:144-193)."""
        log = os.path.join(self.checkpoint_path, "results.txt")
        head = (f"data_size: {data_size}, data_range: {list(data_range)}, batch_size: {batch_size}, epoch: {epoch}, "
                f"valid_freq: {valid_freq}, save_freq: {save_freq}, lr: {lr}, lr_decay: {lr_decay}, decay_freq: {decay_freq}, "
                f"robot_G: {self.G.cpu()}, robot_h: {self.h.cpu()}")
        with open(log, "a") as f:
            print(head + "\n", file=f)
        with open(os.path.join(self.checkpoint_path, "train_dict.pkl"), "wb") as f:
            pickle.dump(dict(data_size=data_size, data_range=list(data_range), batch_size=batch_size, epoch=epoch,
                             valid_freq=valid_freq, save_freq=save_freq, lr=lr, lr_decay=lr_decay, decay_freq=decay_freq), f)
        self.optimizer.param_groups[0]["lr"] = float(lr)
        P, MU, D = self.generate_data_set(data_size, data_range)
        perm = torch.randperm(data_size, device=self.device)            # random_split :191-193
        ntr = int(data_size * 0.8)
        tr, va = perm[:ntr], perm[ntr:ntr + int(data_size * 0.2)]
        return log, (P[tr], MU[tr], D[tr]), (P[va], MU[va], D[va])

    def _log_epoch(self, log, i, epoch, train_losses, valid_losses):
        (ml, dl, al, bl), (vml, vdl, val, vbl) = train_losses, valid_losses
        with open(log, "a") as f:
            print(f"Epoch {i}/{epoch} learning rate {self.optimizer.param_groups[0]['lr']} \n"
                  "---------------------------------\nLosses:\n"
                  f"  Mu Loss:          {ml:.2e}   | Validate Mu Loss:            {vml:.2e}\n"
                  f"  Distance Loss:    {dl:.2e}   | Validate Distance Loss:      {vdl:.2e}\n"
                  f"  Fa Loss:          {al:.2e}   | Validate Fa Loss:            {val:.2e}\n"
                  f"  Fb Loss:          {bl:.2e}   | Validate Fb Loss:            {vbl:.2e}\n", file=f)

    def _after_epoch(self, log, i, save_freq, lr_decay, decay_freq, save_loss, train_losses, full):
        """Checkpoint, learning-rate decay and loss list at the end of epoch i (:270-300); returns the last checkpoint."""
        if i % save_freq == 0:
            full = os.path.join(self.checkpoint_path, f"model_{i}.pth")
            torch.save({k: v.detach().cpu() for k, v in self.model.state_dict().items()}, full)
        if (i + 1) % decay_freq == 0:
            self.optimizer.param_groups[0]["lr"] *= lr_decay
            with open(log, "a") as f:
                print("current learning rate:", self.optimizer.param_groups[0]["lr"], file=f)
        self.loss_list.append(sum(train_losses))
        if save_loss:
            with open(os.path.join(self.checkpoint_path, "loss.pkl"), "wb") as f:
                pickle.dump(self.loss_list, f)
        return full

    def start(self, data_size=100000, data_range=(-25, -25, 25, 25), batch_size=256, epoch=5000, valid_freq=100,
              save_freq=500, lr=5e-5, lr_decay=0.5, decay_freq=1500, save_loss=False, engine="torch", **kwargs):
        """engine="torch": the optimisation is PyTorch autograd, as in the reference.  engine="hip": every training and
        every validation epoch is ONE launch of the fused kernel (csrc/dune_train.hip, include/neupan_amd_train.h); the
        data set, the split, the per-batch rotation angles (same draws in the same order), the log, the checkpoints and
        the learning-rate decay are the same."""
        if engine not in ("torch", "hip"):
            raise ValueError(f"DuneTrain.start: unknown engine {engine!r} (\"torch\" or \"hip\")")
        if engine == "hip":
            _require_default_model(self.model, self.G.shape[0])
        log, train, valid = self._prepare(data_size, data_range, batch_size, epoch, valid_freq, save_freq, lr, lr_decay, decay_freq)
        if engine == "hip":
            return _hip_loop([self], [log], [train], [valid], batch_size, epoch, valid_freq, save_freq, lr_decay, decay_freq,
                             save_loss)[0]
        full = None
        for i in range(epoch + 1):
            self.model.train(True)
            tl = self._epoch(train, batch_size, False)
            if i % valid_freq == 0:
                self.model.eval()
                self._log_epoch(log, i, epoch, tl, self._epoch(valid, batch_size, True))
            full = self._after_epoch(log, i, save_freq, lr_decay, decay_freq, save_loss, tl, full)
        return full


# ---- the hip engine: parameter pack, the epoch launch, several runs side by side -----------------------------------------------

PACK_KEYS = ("MLP.0.weight", "MLP.0.bias", "MLP.1.weight", "MLP.1.bias", "MLP.3.weight", "MLP.3.bias", "MLP.5.weight", "MLP.5.bias",
             "MLP.6.weight", "MLP.6.bias", "MLP.8.weight", "MLP.8.bias", "MLP.10.weight", "MLP.10.bias", "MLP.11.weight",
             "MLP.11.bias", "MLP.13.weight", "MLP.13.bias")


def pack_layout(E):
    """{state_dict key: (offset, shape)} of the parameter pack of ObsPointNet(2, E) (include/neupan_amd_train.h), and its length."""
    shapes = [(32, 2), (32,), (32,), (32,)] + [(32, 32), (32,), (32, 32), (32,), (32,), (32,)] * 2 + [(32, 32), (32,)]
    shapes = shapes[:16] + [(E, 32), (E,)]
    out, off = {}, 0
    for k, sh in zip(PACK_KEYS, shapes):
        out[k] = (off, sh)
        off += int(np.prod(sh))
    return out, off


def _require_default_model(model, E):
    sd = model.state_dict() if isinstance(model, ObsPointNet) else None
    lay, _ = pack_layout(E)
    if sd is None or list(sd.keys()) != list(PACK_KEYS) or any(tuple(sd[k].shape) != lay[k][1] for k in PACK_KEYS):
        raise ValueError(f"engine=\"hip\" trains the default ObsPointNet(2, {E}) only (include/neupan_amd_train.h)")


def pack_params(model):
    """The parameters of an ObsPointNet as one float32 vector [P] in the kernel's order: the state_dict's tensors, flat."""
    sd = model.state_dict()
    return torch.cat([sd[k].detach().reshape(-1).to(torch.float32) for k in PACK_KEYS])


def unpack_params(flat, model):
    """Write a parameter pack back into the model (the inverse of pack_params)."""
    sd = model.state_dict()
    lay, P = pack_layout(sd["MLP.13.bias"].shape[0])
    if flat.numel() != P:
        raise ValueError(f"unpack_params: {flat.numel()} values for a pack of {P}")
    with torch.no_grad():
        for k, (off, sh) in lay.items():
            sd[k].copy_(flat[off:off + int(np.prod(sh))].reshape(sh))
    return model


def train_steps(G, h, points, mu, dist, first_row, batch, rot, params, adam_m=None, adam_v=None, step_count=None, lr=1e-4,
                betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, train=True, grad_out=None, losses=None):
    """npa_dune_train_steps on float32 device tensors: G [R,E,2], h [R,E], points [R,n,2], mu [R,n,E], dist [R,n],
    rot [steps,2], params (and adam_m, adam_v) [R,P], step_count int32 [R].  Returns losses [R,steps,4] (device)."""
    from . import _lib_train
    lib = _lib_train.load()
    R, E = G.shape[0], G.shape[1]
    steps, n = rot.shape[0], points.shape[1]
    P = lib.npa_dune_train_param_count(E)
    for name, t, shape in (("G", G, (R, E, 2)), ("h", h, (R, E)), ("points", points, (R, n, 2)), ("mu", mu, (R, n, E)),
                           ("dist", dist, (R, n)), ("rot", rot, (steps, 2)), ("params", params, (R, P)), ("adam_m", adam_m, (R, P)),
                           ("adam_v", adam_v, (R, P)), ("grad_out", grad_out, (R, P)), ("losses", losses, (R, steps, 4))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
            raise ValueError(f"train_steps: {name} must be a contiguous float32 device tensor of shape {shape}")
    if step_count is not None and (tuple(step_count.shape) != (R,) or step_count.dtype != torch.int32 or not step_count.is_cuda):
        raise ValueError("train_steps: step_count must be an int32 device tensor of shape (runs,)")
    if losses is None:
        losses = torch.empty((R, steps, 4), dtype=torch.float32, device=params.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(params.device):
        rc = lib.npa_dune_train_steps(R, E, ptr(G), ptr(h), n, ptr(points), ptr(mu), ptr(dist), int(first_row), int(batch), steps,
                                      ptr(rot), lr, betas[0], betas[1], eps, weight_decay, 1 if train else 0, ptr(params),
                                      ptr(adam_m), ptr(adam_v), ptr(step_count), ptr(losses), ptr(grad_out),
                                      torch.cuda.current_stream().cuda_stream)
    _lib_train.check(rc, "npa_dune_train_steps")
    return losses


def _hip_epoch(state, data, batch_size, validate, group):
    """One epoch = one launch; the angles are drawn as DuneTrain._epoch draws them.  Returns [R,4] epoch means (float64)."""
    P, MU, D = data
    steps = -(-P.shape[1] // batch_size)
    th = np.array([np.random.uniform(0, 2 * np.pi) for _ in range(steps)])
    rot = torch.from_numpy(np.stack([np.cos(th), np.sin(th)], axis=1).astype(np.float32)).to(P.device)
    losses = train_steps(state["G"], state["h"], P, MU, D, 0, batch_size, rot, state["params"], state["m"], state["v"], state["t"],
                         lr=group["lr"], betas=group["betas"], eps=group["eps"], weight_decay=group["weight_decay"],
                         train=not validate)
    return losses.cpu().numpy().astype(np.float64).sum(axis=1) / steps          # (the one read-back of the epoch)


def _hip_loop(trainers, logs, trains, valids, batch_size, epoch, valid_freq, save_freq, lr_decay, decay_freq, save_loss):
    """The epoch loop of DuneTrain.start for R trainers side by side (one workgroup each): same log, checkpoints and decay."""
    dev = trainers[0].device
    stack = lambda sets, k: torch.stack([s[k] for s in sets]).contiguous()
    train, valid = tuple(stack(trains, k) for k in range(3)), tuple(stack(valids, k) for k in range(3))
    params = torch.stack([pack_params(t.model) for t in trainers]).to(dev).contiguous()
    state = dict(G=torch.stack([t.G for t in trainers]).contiguous(), h=torch.stack([t.h.reshape(-1) for t in trainers]).contiguous(),
                 params=params, m=torch.zeros_like(params), v=torch.zeros_like(params),
                 t=torch.zeros(len(trainers), dtype=torch.int32, device=dev))
    fulls = [None] * len(trainers)
    for i in range(epoch + 1):
        group = trainers[0].optimizer.param_groups[0]
        tl = _hip_epoch(state, train, batch_size, False, group)
        if i % valid_freq == 0:
            vl = _hip_epoch(state, valid, batch_size, True, group)
            for r, t in enumerate(trainers):
                t._log_epoch(logs[r], i, epoch, tuple(tl[r]), tuple(vl[r]))
        if i % save_freq == 0 or i == epoch:
            for r, t in enumerate(trainers):
                unpack_params(state["params"][r], t.model)
        for r, t in enumerate(trainers):
            fulls[r] = t._after_epoch(logs[r], i, save_freq, lr_decay, decay_freq, save_loss, tuple(tl[r]), fulls[r])
    return fulls


def train_many(G_list, h_list, checkpoint_paths, seeds=0, device="cuda", **start_kwargs):
    """Train R robots of the same edge count (or R seeds of one robot) side by side with the hip engine: one workgroup per
    run in every launch, one checkpoint directory each.  Run r is set up under seeds[r] (an int: the same for all) exactly
    as `torch.manual_seed(s); np.random.seed(s); DuneTrain(None, G, h, path).start(engine="hip", ...)` sets itself up; the
    rotation angles are one sequence for all runs, continued from run 0's random state, so every run whose seed is run 0's
    gets the bits of that robot trained alone.  Returns the trainers and their last checkpoints."""
    R = len(G_list)
    if not (R >= 1 and len(h_list) == R and len(checkpoint_paths) == R):
        raise ValueError("train_many: G_list, h_list and checkpoint_paths must have the same length >= 1")
    seeds = [seeds] * R if isinstance(seeds, int) else list(seeds)
    if len(seeds) != R:
        raise ValueError("train_many: one seed per run")
    kw = dict(data_size=100000, data_range=(-25, -25, 25, 25), batch_size=256, epoch=5000, valid_freq=100, save_freq=500, lr=5e-5,
              lr_decay=0.5, decay_freq=1500)
    save_loss = start_kwargs.pop("save_loss", False)
    if start_kwargs.pop("engine", "hip") != "hip":
        raise ValueError("train_many runs the hip engine")
    kw.update({k: v for k, v in start_kwargs.items() if k in kw})
    trainers, logs, trains, valids, np_state = [], [], [], [], None
    for r in range(R):
        torch.manual_seed(seeds[r])
        np.random.seed(seeds[r])
        t = DuneTrain(None, G_list[r], h_list[r], checkpoint_paths[r], device=device)
        if trainers and t.G.shape != trainers[0].G.shape:
            raise ValueError("train_many: every robot must have the same number of edges")
        log, tr, va = t._prepare(**kw)
        if r == 0:
            np_state = np.random.get_state()
        trainers.append(t); logs.append(log); trains.append(tr); valids.append(va)
    np.random.set_state(np_state)
    fulls = _hip_loop(trainers, logs, trains, valids, kw["batch_size"], kw["epoch"], kw["valid_freq"], kw["save_freq"],
                      kw["lr_decay"], kw["decay_freq"], save_loss)
    return trainers, fulls
