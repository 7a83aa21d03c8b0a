"""Host-fed serving loop: a packed ragged input record per step and a pipelined upload (include/neupan_amd.h, "the
packed input record"; csrc/ingest.hip).

The reference's contract is neupan.forward(state, points): the cloud arrives from the host on every control cycle
(neupan/neupan.py:123-127).  `InputPipeline` carries a cycle's inputs to the device as ONE record -- header, the dense
nominal / reference tensors and the ragged clouds back to back, only the bytes in use -- on a copy stream of its own,
into a spare device buffer, while the previous cycle still computes; `npa_ingest_unpack`, launched on the step's stream in
front of the step's kernels, moves it into the tensors the step reads.

    pipe = InputPipeline(pan, batch=B, n_stride=N)
    rec = pipe.acquire(); rec.pack(nom_s, nom_u, ref_s, ref_us, clouds); pipe.submit(rec)     # the first cycle's inputs
    step = pipe.make_step(reset_state=True)         # primes the planner on that record
    while serving:
        rec = pipe.acquire()                        # blocks only while THIS host record's last upload is in flight
        rec.pack(...)                               # or write rec.nom_s[...], rec.cloud[...] in place, then rec.seal()
        pipe.submit(rec)                            # one async copy on the copy stream
        out = step()                                # waits for the upload on the device, unpacks, plans
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import NeupanAmdError, check

INT32_MAX = 2 ** 31 - 1
_SECTIONS = ("n_points", "cloud_off", "nom_s", "nom_u", "ref_s", "ref_us", "cloud")


class RecordLayout:
    """Section offsets of a record, as the library lays it out (npa_ingest_layout): `offsets[name]` in bytes for name in
    n_points, cloud_off, nom_s, nom_u, ref_s, ref_us, cloud; `total_bytes` = a record whose every cloud is n_stride long."""

    def __init__(self, batch, receding, n_stride, velocities=False):
        self.batch, self.T, self.n_stride, self.velocities = int(batch), int(receding), int(n_stride), bool(velocities)
        self.comps = 4 if self.velocities else 2
        out = (C.c_size_t * 8)()
        check(_lib.load().npa_ingest_layout(self.batch, self.T, self.n_stride, int(self.velocities), out, 8), "npa_ingest_layout")
        self.offsets = {k: int(out[i]) for i, k in enumerate(_SECTIONS)}
        self.total_bytes = int(out[7])
        B, T = self.batch, self.T
        self.shapes = dict(n_points=(B,), cloud_off=(B,), nom_s=(B, 3, T + 1), nom_u=(B, 2, T), ref_s=(B, 3, T + 1), ref_us=(B, T),
                           cloud=(B * self.n_stride * self.comps,))


class HostRecord:
    """One record in host memory: `words` (int32, the whole buffer) and typed numpy VIEWS of its sections -- n_points,
    cloud_off (int32), nom_s, nom_u, ref_s, ref_us (float32, npa_forward_batch's shapes) and cloud (float32, flat: the
    cloud section).  Fill it with pack(), or write the views in place and call seal().  `used_bytes` is what has to be
    uploaded: everything up to the last cloud word in use.  words=None allocates plain host memory (tools, tests); an
    InputPipeline hands out records that live in pinned memory."""

    def __init__(self, layout, words=None, slot=None):
        self.layout, self.slot = layout, slot
        nw = layout.total_bytes // 4
        if words is None:
            words = np.zeros(nw, dtype=np.int32)
        if words.dtype != np.int32 or words.shape != (nw,) or not words.flags["C_CONTIGUOUS"]:
            raise ValueError(f"HostRecord: the buffer must be {nw} contiguous int32 words")
        self.words = words
        for k in _SECTIONS:
            o, shape = layout.offsets[k] // 4, layout.shapes[k]
            v = words[o:o + int(np.prod(shape))]
            setattr(self, k, (v if k in ("n_points", "cloud_off") else v.view(np.float32)).reshape(shape))
        self.used_bytes = layout.offsets["cloud"]

    def seal(self):
        """After writing the views in place: work out used_bytes from the header (the furthest cloud word a scene owns).
        A header that points outside the cloud section is not refused here -- the device rejects such scenes
        (InputPipeline.status) -- but never makes the upload longer than the record."""
        lay = self.layout
        n, off = self.n_points.astype(np.int64), self.cloud_off.astype(np.int64)
        end = int(np.max(np.where(n > 0, off + lay.comps * n, 0), initial=0))
        self.used_bytes = min(lay.offsets["cloud"] + 4 * max(end, 0), lay.total_bytes)
        return self.used_bytes

    def pack(self, nom_s, nom_u, ref_s, ref_us, clouds, velocities=None):
        """The dense tensors (npa_forward_batch's shapes) and one (2, n_b) array per scene, n_b <= n_stride (velocities: the
        same shapes, required exactly when the record carries them).  Clouds are written back to back, cloud_off = the
        exclusive prefix sums; returns used_bytes."""
        lay = self.layout
        B = lay.batch
        for k, a in (("nom_s", nom_s), ("nom_u", nom_u), ("ref_s", ref_s), ("ref_us", ref_us)):
            a = np.asarray(a)
            if a.shape != lay.shapes[k]:
                raise ValueError(f"HostRecord.pack: {k} must have shape {lay.shapes[k]}, got {a.shape}")
            getattr(self, k)[...] = a
        if len(clouds) != B:
            raise ValueError(f"HostRecord.pack: {B} clouds expected, got {len(clouds)}")
        if (velocities is not None) != lay.velocities:
            raise ValueError("HostRecord.pack: velocities must be given exactly when the record was laid out with them")
        if velocities is not None and len(velocities) != B:
            raise ValueError(f"HostRecord.pack: {B} velocity arrays expected, got {len(velocities)}")
        off = 0
        for b in range(B):
            c = np.asarray(clouds[b])
            if c.ndim != 2 or c.shape[0] != 2:
                raise ValueError(f"HostRecord.pack: cloud {b} must have shape (2, n), got {c.shape}")
            n = c.shape[1]
            if n > lay.n_stride:
                raise ValueError(f"HostRecord.pack: cloud {b} has {n} points, the stride is {lay.n_stride}")
            self.n_points[b], self.cloud_off[b] = n, off
            self.cloud[off:off + 2 * n] = c.reshape(-1)
            if velocities is not None:
                v = np.asarray(velocities[b])
                if v.shape != c.shape:
                    raise ValueError(f"HostRecord.pack: velocities {b} must have the cloud's shape {c.shape}, got {v.shape}")
                self.cloud[off + 2 * n:off + 4 * n] = v.reshape(-1)
            off += lay.comps * n
        self.used_bytes = lay.offsets["cloud"] + 4 * off
        return self.used_bytes


_copy_streams = {}


def copy_stream(device):
    """THE copy stream of `device` for this process: every pipeline and every slot shares it (the device schedules a limited
    number of hardware queues per process and the compute chains own them; uploads are serial on the
    link anyway)."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _copy_streams.get(idx)
    if st is None:
        st = _copy_streams[idx] = torch.cuda.Stream(device=idx)
    return st


class InputPipeline:
    """`depth` pinned host records, `depth` device record buffers, ONE set of unpacked input tensors (nom_s, nom_u, ref_s,
    ref_us, points (B, 2, n_stride), velocities | None, n_points) and the events that order them.  Records are consumed in
    the order they were submitted, one per step().  Nothing here synchronises the host with the device except acquire()
    (only while the record it is about to hand out is still being uploaded) and status()."""

    def __init__(self, pan, batch, n_stride, velocities=False, depth=2):
        if depth < 1:
            raise ValueError("InputPipeline: depth >= 1")
        self.pan, self.device, self.depth = pan, pan.device, int(depth)
        self.layout = lay = RecordLayout(batch, pan.T, n_stride, velocities)
        self._lib = _lib.load()
        dev, B, T = self.device, lay.batch, lay.T
        nw = lay.total_bytes // 4
        self._host = [torch.zeros(nw, dtype=torch.int32).pin_memory() for _ in range(self.depth)]
        self._records = [HostRecord(lay, h.numpy(), slot=r) for r, h in enumerate(self._host)]
        self._dev = [torch.zeros(nw, dtype=torch.int32, device=dev) for _ in range(self.depth)]
        f32 = dict(dtype=torch.float32, device=dev)
        self.nom_s, self.nom_u = torch.zeros((B, 3, T + 1), **f32), torch.zeros((B, 2, T), **f32)
        self.ref_s, self.ref_us = torch.zeros((B, 3, T + 1), **f32), torch.zeros((B, T), **f32)
        self.points = torch.zeros((B, 2, lay.n_stride), **f32)
        self.velocities = torch.zeros((B, 2, lay.n_stride), **f32) if lay.velocities else None
        self.n_points = torch.zeros((B,), dtype=torch.int32, device=dev)
        self._status = torch.tensor([0, INT32_MAX], dtype=torch.int32, device=dev)
        self._copy = copy_stream(dev)
        for t in self._dev:
            t.record_stream(self._copy)
        self._uploaded = [torch.cuda.Event() for _ in range(self.depth)]     # "the upload of slot r has landed"
        self._free = [torch.cuda.Event() for _ in range(self.depth)]         # "device record r has been unpacked"
        self._uploading = [False] * self.depth       # an upload of slot r was issued and acquire() has not waited for it yet
        self._freed = [False] * self.depth           # _free[r] has been recorded at least once
        self._pending = collections.deque()          # (slot, bytes) submitted and not yet consumed by a step
        self._next = 0
        self._step = None
        self._args = (B, T, lay.n_stride, int(lay.velocities))
        self._outs = tuple(C.c_void_p(t.data_ptr()) if t is not None else None for t in
                           (self.nom_s, self.nom_u, self.ref_s, self.ref_us, self.points, self.velocities, self.n_points, self._status))
        self._idx = dev.index if dev.index is not None else torch.cuda.current_device()
        torch.cuda.current_stream(dev).synchronize()  # (once: the zero fills above, before another stream touches the buffers)

    # ------------------------------------------------------------------ host side
    def acquire(self):
        """The next host record (round robin).  Blocks only while that record's previous upload is still in flight."""
        r = self._next
        if self._uploading[r]:
            self._uploaded[r].synchronize()
            self._uploading[r] = False
        self._next = (r + 1) % self.depth
        return self._records[r]

    def submit(self, rec):
        """Upload `rec` (only rec.used_bytes of it) on the copy stream, behind "device record r has been unpacked"."""
        r = rec.slot
        if r is None or rec is not self._records[r]:
            raise NeupanAmdError("InputPipeline.submit: not a record of this pipeline (acquire() hands them out)")
        if any(s == r for s, _ in self._pending):
            raise NeupanAmdError(f"InputPipeline.submit: record {r} was submitted and no step has consumed it yet "
                                 f"(depth {self.depth}: at most that many submits ahead of the steps)")
        lay = self.layout
        nbytes = int(rec.used_bytes)
        if nbytes % 4 or not lay.offsets["cloud"] <= nbytes <= lay.total_bytes:
            raise NeupanAmdError(f"InputPipeline.submit: used_bytes {nbytes} outside [{lay.offsets['cloud']}, {lay.total_bytes}]")
        cp = self._copy
        with torch.cuda.stream(cp):
            if self._freed[r]:
                cp.wait_event(self._free[r])
            self._dev[r][:nbytes // 4].copy_(self._host[r][:nbytes // 4], non_blocking=True)
            self._uploaded[r].record(cp)
        self._uploading[r] = True
        self._pending.append((r, nbytes))
        return nbytes

    # ------------------------------------------------------------------ device side
    def _consume(self):
        """On the CURRENT stream: wait for the oldest submitted record's upload, unpack it, release its device buffer."""
        if not self._pending:
            raise NeupanAmdError("InputPipeline: step() without a submitted record (acquire / pack / submit one per step)")
        r, nbytes = self._pending.popleft()
        dev = self.device
        st = torch.cuda.current_stream(dev)
        st.wait_event(self._uploaded[r])
        call = lambda: self._lib.npa_ingest_unpack(*self._args, C.c_void_p(self._dev[r].data_ptr()), nbytes, *self._outs,
                                                   C.c_void_p(st.cuda_stream))
        if torch.cuda.current_device() != self._idx:     # the launch must see the device of the buffers
            with torch.cuda.device(dev):
                rc = call()
        else:
            rc = call()
        if rc:
            check(rc, "npa_ingest_unpack")
        self._free[r].record(st)
        self._freed[r] = True

    def make_step(self, **kw):
        """PAN.make_step on the pipeline's unpacked tensors (keywords: reset_state, out_u, reset_every_step), with the unpack
        installed as the step's pre_issue: every step() -- alone, or as a member of a StepGroup / StepLoop, which run
        pre_issue under the member's stream -- consumes one submitted record.  make_step itself plans once (PAN.make_step
        primes the planner): on the record submitted before this call, which it consumes, or on empty inputs (zeros, no
        points) when there is none.  One step per pipeline; graph=True raises (a captured step has no pre_issue)."""
        if kw.get("graph"):
            raise NeupanAmdError("InputPipeline.make_step: graph=True is not supported (a captured step runs no pre_issue, "
                                 "so nothing would wait for the upload or unpack it)")
        bad = set(kw) - {"reset_state", "out_u", "reset_every_step", "graph"}
        if bad:
            raise TypeError(f"InputPipeline.make_step: unexpected arguments {sorted(bad)} (the inputs are the pipeline's)")
        if self._step is not None:
            raise NeupanAmdError("InputPipeline.make_step: this pipeline already feeds a step (one set of input tensors)")
        if self._pending:
            self._consume()
        step = self.pan.make_step(self.nom_s, self.nom_u, self.ref_s, self.ref_us, self.points, self.velocities, self.n_points, **kw)
        step.pre_issue = self._consume
        self._step = step
        return step

    def status(self, reset=False):
        """(scenes rejected by the unpack so far, smallest rejected scene index or -1).  Synchronises the device."""
        torch.cuda.synchronize(self.device)
        n, first = (int(v) for v in self._status.cpu())
        if reset:
            self._status.copy_(torch.tensor([0, INT32_MAX], dtype=torch.int32))
            torch.cuda.synchronize(self.device)
        return n, (first if n else -1)
