"""CPU tests of the host / device marshalling in pesto_amd._lib (Side, put, check): no GPU, the library replaced by a recorder."""
import numpy as np
import pytest

from pesto_amd import _lib


class _Recorder:
    """Stands in for libpesto_hip.so: every entry point returns 0 and is recorded."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return b"recorded message" if name.endswith("last_error") else 0
        return f


class _RocmLike:
    """Looks like a ROCm tensor to Side (is_cuda, device) without a GPU."""
    is_cuda = True

    def __init__(self, index, shape=(4, 3)):
        import torch
        self.device = torch.device("cuda", index)
        self.shape = shape

    def detach(self):
        return self


@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    return rec


@pytest.fixture
def model(lib):
    from pesto_amd import Model
    from pesto_amd.config import CONFIGS
    from pesto_amd.weights import blob_size
    m = Model(CONFIGS["i_v4_0"])
    m.load_blob(np.zeros(blob_size(m.config), np.float32))
    yield m
    m._handle = None                # (the recorder made no handle)


def _device_side(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": 1234})())
    return _lib.Side(_RocmLike(0), 0)


def test_put_coerces_dtype_and_layout():
    import torch
    side = _lib.Side(np.zeros((4, 3)), 0)
    assert side.device is None and side.stream is None and side.kind == _lib.PTR_HOST
    a = np.arange(24, dtype=np.float64).reshape(4, 6)[:, ::2]
    out = side.put(a, np.float32, (4, 3))
    assert out.dtype == np.float32 and out.flags.c_contiguous and np.array_equal(out, a)
    same = np.zeros((4, 3), np.float32)
    assert side.put(same, np.float32) is same                          # nothing to do: no copy
    assert side.put([[1, 2, 3]], np.int32).dtype == np.int32
    t = torch.arange(6, dtype=torch.int16).reshape(2, 3)
    out = side.put(t, (np.int64, np.int32))
    assert isinstance(out, np.ndarray) and out.dtype == np.int64 and _lib.ids_kind(out) == _lib.IDS_INT64
    out = side.put(t.to(torch.int32), (np.int64, np.int32))
    assert out.dtype == np.int32 and _lib.ids_kind(out) == _lib.IDS_INT32
    assert side.put(np.array([-1], np.int64), np.uint32)[0] == 0xffffffff
    with pytest.raises(ValueError, match="X must be"):
        side.put(np.zeros((5, 3)), np.float32, (4, 3), "X")


def test_put_strided_keeps_a_view_with_a_contiguous_row():
    side = _lib.Side(np.zeros(1), 0)
    traj = np.zeros((10, 4, 3), np.float32)                              # [N, F, 3]
    v = side.put(traj.transpose(1, 0, 2), np.float32, strided=True)      # read in place
    assert np.shares_memory(v, traj) and _lib.strides(v) == (3, 12, 1)
    c = side.put(traj[:, :, ::-1], np.float32, strided=True)             # no contiguous row: copied
    assert not np.shares_memory(c, traj) and c.flags.c_contiguous
    assert _lib.strides(side.put(traj.astype(np.float64), np.float32, strided=True)) == (12, 3, 1)


def test_cat_and_empty_on_the_host():
    side = _lib.Side([], 0)
    out = side.cat([np.ones((2, 3), np.float64), [[0, 0, 0]]], np.float32)
    assert out.dtype == np.float32 and out.shape == (3, 3) and out.flags.c_contiguous
    e = side.empty((2, 5), np.int32)
    assert isinstance(e, np.ndarray) and e.dtype == np.int32 and e.shape == (2, 5)
    assert side.ptr(e) == e.ctypes.data and side.ptr(None) is None


def test_host_side_refuses_tensors_in_ptr():
    import torch
    with pytest.raises(RuntimeError):
        _lib.Side(np.zeros(1), 0).ptr(torch.zeros(3))


def test_device_side_refuses_host_arrays_without_a_library_call(monkeypatch, lib):
    import torch
    side = _device_side(monkeypatch)
    assert side.kind == _lib.PTR_DEVICE and side.stream == 1234 and side.device == torch.device("cuda", 0)
    for a in (torch.zeros(3), np.zeros(3, np.float32)):
        with pytest.raises(RuntimeError):
            side.ptr(a)
    assert lib.calls == []


def test_device_lead_on_another_gpu_raises_in_every_entry_point(model, lib):
    from pesto_amd.evaluate import bc_scores_batch, contact_labels
    from pesto_amd.patches import patch_labels
    X = _RocmLike(1)
    ids, q, roa = np.zeros((4, 64), np.int64), np.zeros((4, 30), np.float32), np.zeros(4, np.int32)
    calls = [lambda: model.forward_segments(X, ids, q, roa, 1),
             lambda: model.forward_frames_segments(_RocmLike(1, (1, 4, 3)), ids, q, roa, 1),
             lambda: model.postprocess(_RocmLike(1, (2, 5))),
             lambda: model.knn_collate(X, [4]),
             lambda: model.knn_tie_rows(X, [4], ids),
             lambda: model(X, ids, q, _RocmLike(1, (4, 1))),
             lambda: contact_labels(model, X, roa, roa, roa, roa, [4], 1),
             lambda: bc_scores_batch(model, [np.zeros((2, 5))], [_RocmLike(1, (2, 5))]),
             lambda: patch_labels(model, [_RocmLike(1, (2, 5))], [np.zeros((2, 3))])]
    for call in calls:
        with pytest.raises(RuntimeError, match="cuda:1"):
            call()
    assert [name for name, _ in lib.calls if name != "pesto_create"] == []


def test_check_reads_the_error_function_it_is_given(lib):
    _lib.check(0, lambda: pytest.fail("read on success"))
    with pytest.raises(_lib.PestoError, match="eval channel") as e:
        _lib.check(-3, lambda: b"eval channel")
    assert e.value.code == -3
    with pytest.raises(_lib.PestoError, match="recorded message") as e:
        _lib.check(-2)                                                  # default: pesto_last_error
    assert e.value.code == -2 and lib.calls[-1][0] == "pesto_last_error"


def _last(lib, name):
    args = [a for n, a in lib.calls if n == name]
    assert len(args) == 1, (name, lib.calls)
    assert args[0][-2:] == (_lib.PTR_HOST, None)                        # host pointers, no stream
    return args[0]


@pytest.mark.parametrize("lead", ["numpy", "cpu_tensor"])
def test_host_return_types(model, lib, lead):
    import torch
    from pesto_amd.evaluate import bc_scores_batch, contact_labels
    from pesto_amd.patches import patch_labels
    kind = (lambda a: torch.from_numpy(np.asarray(a))) if lead == "cpu_tensor" else np.asarray
    like = torch.Tensor if lead == "cpu_tensor" else np.ndarray
    N, R, C = 6, 2, model.config["dm"]["N2"]
    X, q = kind(np.zeros((N, 3), np.float32)), kind(np.zeros((N, 30), np.float32))
    ids, roa = kind(np.zeros((N, 64), np.int32)), kind(np.zeros(N, np.int32))

    z = model.forward_segments(X, ids, q, roa, R)
    assert isinstance(z, like) and tuple(z.shape) == (R, C)
    assert _last(lib, "pesto_forward")[6] == _lib.IDS_INT32
    z = model.forward_segments(X, ids, q, roa, R, sizes=[2, 4])
    assert isinstance(z, like) and _last(lib, "pesto_forward_structures")[4] == 2
    zf = model.forward_frames_segments(kind(np.zeros((3, N, 3), np.float32)), ids, q, roa, R)
    assert isinstance(zf, like) and tuple(zf.shape) == (3, R, C)
    _last(lib, "pesto_forward_frames")
    p, bf = model.postprocess(z, roa)
    assert isinstance(p, like) and isinstance(bf, like) and tuple(bf.shape) == (C, N)
    assert model.postprocess(z)[1] is None
    k = model.knn_collate(X, [2, 4])
    assert isinstance(k, like) and k.dtype in (np.int64, torch.int64)
    fl = model.knn_tie_rows(X, [2, 4], ids)
    assert isinstance(fl, np.ndarray) and fl.dtype == np.uint8 and fl.shape == (N,)
    labels, ties = contact_labels(model, X, roa, roa, roa, roa, [N], 3)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.uint32 and ties.dtype == np.uint8
    sc = bc_scores_batch(model, [kind(np.zeros((R, 2), np.float32))], [kind(np.zeros((R, 2), np.float32))])
    assert isinstance(sc, like) and tuple(sc.shape) == (1, 8, 2)
    out = patch_labels(model, [kind(np.zeros((R, 2), np.float32))], [kind(np.zeros((R, 3), np.float32))])
    assert all(isinstance(o, np.ndarray) for o in out)
    for name in ("pesto_postprocess", "pesto_knn_collate", "pesto_knn_tie_rows", "pesto_interface_labels", "pesto_bc_scores",
                 "pesto_interface_patches"):
        assert any(n == name and a[-2:] == (_lib.PTR_HOST, None) for n, a in lib.calls), name
