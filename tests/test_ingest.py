"""CPU tests of the packed input record (include/neupan_amd.h, neupan_amd/ingest.py): the symbols, the layout the library owns,
and the host-side packer against an unpack written here in numpy."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from neupan_amd import build
    build.build(force=False, verbose=False)
    from neupan_amd import _lib
    return _lib.load()


def test_ingest_symbols_resolve(lib):
    from neupan_amd import _lib
    for name in ("npa_ingest_layout", "npa_ingest_unpack"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    # argument errors are answered on the host, before anything touches a device
    out = (C.c_size_t * 8)()
    assert lib.npa_ingest_layout(0, 10, 100, 0, out, 8) == -1 and lib.npa_ingest_layout(4, 10, 100, 0, None, 8) == -1
    assert lib.npa_ingest_layout(4, 10, 100, 0, out, 9) == -1 and lib.npa_ingest_layout(4, 22, 100, 0, out, 8) == -1
    assert lib.npa_ingest_layout(1 << 20, 10, 1 << 10, 1, out, 8) == -1          # 2^32 cloud words: no int32 offset reaches them
    assert lib.npa_ingest_unpack(4, 10, 100, 0, None, 0, *([None] * 8), None) == -1
    assert b"npa_ingest_unpack" in lib.npa_last_error()


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [10, 20])
@pytest.mark.parametrize("vel", [False, True])
def test_layout_sections_are_aligned_and_disjoint(lib, B, T, vel):
    n_stride = 130
    out = (C.c_size_t * 8)()
    assert lib.npa_ingest_layout(B, T, n_stride, int(vel), out, 8) == 0
    off, total = list(out)[:7], out[7]
    words = [B, B, B * 3 * (T + 1), B * 2 * T, B * 3 * (T + 1), B * T, B * n_stride * (4 if vel else 2)]
    assert off[0] == 0
    for i in range(7):
        assert off[i] % 256 == 0
        end = off[i] + 4 * words[i]
        assert end <= (off[i + 1] if i < 6 else total), (i, off, total)       # in order, not overlapping, inside the total
    assert total % 256 == 0 and total - (off[6] + 4 * words[6]) < 256          # no slack beyond the alignment
    short = (C.c_size_t * 3)()
    assert lib.npa_ingest_layout(B, T, n_stride, int(vel), short, 3) == 0 and list(short) == off[:3]
    from neupan_amd.ingest import RecordLayout
    lay = RecordLayout(B, T, n_stride, vel)
    assert [lay.offsets[k] for k in ("n_points", "cloud_off", "nom_s", "nom_u", "ref_s", "ref_us", "cloud")] == off
    assert lay.total_bytes == total and lay.comps == (4 if vel else 2)


def numpy_unpack(lay, words, used_bytes):
    """The record format, restated: reads ONLY words[:used_bytes / 4]."""
    w = np.array(words[:used_bytes // 4])                   # (a copy cut at the upload's length: a read beyond it raises)
    B, T, N = lay.batch, lay.T, lay.n_stride
    sec = lambda k, n: w[lay.offsets[k] // 4: lay.offsets[k] // 4 + n]
    out = dict(n_points=sec("n_points", B).copy(), cloud_off=sec("cloud_off", B).copy(),
               nom_s=sec("nom_s", B * 3 * (T + 1)).view(np.float32).reshape(B, 3, T + 1),
               nom_u=sec("nom_u", B * 2 * T).view(np.float32).reshape(B, 2, T),
               ref_s=sec("ref_s", B * 3 * (T + 1)).view(np.float32).reshape(B, 3, T + 1),
               ref_us=sec("ref_us", B * T).view(np.float32).reshape(B, T))
    cloud = w[lay.offsets["cloud"] // 4:].view(np.float32)
    out["clouds"], out["velocities"] = [], []
    for b in range(B):
        n, o = int(out["n_points"][b]), int(out["cloud_off"][b])
        assert o + lay.comps * n <= cloud.size
        out["clouds"].append(cloud[o:o + 2 * n].reshape(2, n))
        if lay.velocities:
            out["velocities"].append(cloud[o + 2 * n:o + 4 * n].reshape(2, n))
    return out


@pytest.mark.parametrize("vel", [False, True])
def test_packer_round_trips_through_a_numpy_unpack(lib, vel):
    from neupan_amd.ingest import HostRecord, RecordLayout
    B, T, N = 5, 10, 37
    lay = RecordLayout(B, T, N, vel)
    rec = HostRecord(lay)
    rec.words[:] = -1                                        # stale content of an earlier cycle
    rng = np.random.default_rng(3)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    dense = dict(nom_s=f(B, 3, T + 1), nom_u=f(B, 2, T), ref_s=f(B, 3, T + 1), ref_us=f(B, T))
    ns = [0, 1, N, 0, 12]
    clouds = [f(2, n) for n in ns]
    vels = [f(2, n) for n in ns] if vel else None
    used = rec.pack(dense["nom_s"], dense["nom_u"], dense["ref_s"], dense["ref_us"], clouds, vels)
    c = lay.comps
    assert list(rec.n_points) == ns
    assert list(rec.cloud_off) == [int(v) for v in np.concatenate([[0], np.cumsum([c * n for n in ns])[:-1]])]   # exclusive prefix sums
    assert used == rec.used_bytes == lay.offsets["cloud"] + 4 * c * sum(ns) < lay.total_bytes                     # only the bytes in use
    got = numpy_unpack(lay, rec.words, used)
    for k, v in dense.items():
        np.testing.assert_array_equal(got[k].view(np.uint32), v.view(np.uint32))
    for b in range(B):
        np.testing.assert_array_equal(got["clouds"][b].view(np.uint32), clouds[b].view(np.uint32))
        if vel:
            np.testing.assert_array_equal(got["velocities"][b].view(np.uint32), vels[b].view(np.uint32))
    # the same record written through the field views in place, then sealed
    rec2 = HostRecord(lay)
    for k, v in dense.items():
        getattr(rec2, k)[...] = v
    rec2.n_points[:], rec2.cloud_off[:] = rec.n_points, rec.cloud_off
    rec2.cloud[:c * sum(ns)] = rec.cloud[:c * sum(ns)]
    assert rec2.seal() == used
    got2 = numpy_unpack(lay, rec2.words, used)              # (the alignment gaps between sections carry no meaning)
    for k in ("n_points", "cloud_off", "nom_s", "nom_u", "ref_s", "ref_us"):
        np.testing.assert_array_equal(got2[k].view(np.uint32), got[k].view(np.uint32))
    for b in range(B):
        np.testing.assert_array_equal(got2["clouds"][b].view(np.uint32), clouds[b].view(np.uint32))
    # every cloud at the stride: the worst case the layout sizes the buffer for
    full = [f(2, N) for _ in range(B)]
    assert rec.pack(dense["nom_s"], dense["nom_u"], dense["ref_s"], dense["ref_us"], full, full if vel else None) \
        == lay.offsets["cloud"] + 4 * c * B * N <= lay.total_bytes


def test_pack_refuses_what_does_not_fit(lib):
    from neupan_amd.ingest import HostRecord, RecordLayout
    B, T, N = 2, 10, 16
    lay = RecordLayout(B, T, N, False)
    rec = HostRecord(lay)
    z = lambda *s: np.zeros(s, dtype=np.float32)
    dense = (z(B, 3, T + 1), z(B, 2, T), z(B, 3, T + 1), z(B, T))
    with pytest.raises(ValueError, match="stride"):
        rec.pack(*dense, [z(2, 3), z(2, N + 1)])
    with pytest.raises(ValueError):
        rec.pack(*dense, [z(2, 3)])                                     # one cloud short
    with pytest.raises(ValueError):
        rec.pack(*dense, [z(2, 3), z(3, 3)])                            # not (2, n)
    with pytest.raises(ValueError):
        rec.pack(z(B, 3, T), *dense[1:], [z(2, 3), z(2, 3)])            # nom_s of another horizon
    with pytest.raises(ValueError):
        rec.pack(*dense, [z(2, 3), z(2, 3)], [z(2, 3), z(2, 3)])        # velocities for a record laid out without them
    recv = HostRecord(RecordLayout(B, T, N, True))
    with pytest.raises(ValueError):
        recv.pack(*dense, [z(2, 3), z(2, 3)])                           # ... and none for one laid out with them
    with pytest.raises(ValueError):
        recv.pack(*dense, [z(2, 3), z(2, 3)], [z(2, 3), z(2, 4)])
