"""HDF5 result store: what the reference's bulk driver writes, ``hf[key] = p.cpu().numpy()`` per structure into
``h5py.File(output_filepath, 'w')`` (interfaceome/apply_model.py:53-79) - one plain (contiguous, unfiltered) dataset per key, the
``/`` in a key creating the groups on the way, exactly as h5py does.

h5py is not a dependency of this package; the HDF5 C library is bound directly with ctypes (the 1.10 / 1.12 / 1.14 C API used here is
the same: H5Fcreate / H5Dcreate2 / H5Dwrite / H5Dread; the link visitor is exported as H5Lvisit by 1.10 and as H5Lvisit2 / H5Lvisit1
from 1.12 on, where H5Lvisit is a header macro - it is resolved lazily, by keys() only, so writing never depends on it. hid_t is
bound as int64: the 1.10+ ABI). The library is looked for in ``$PESTO_HDF5_LIB``, the loader's
search path and the usual prefixes (``/opt/conda/lib`` in the ROCm image). No library -> H5Unavailable with the places that were tried:
the caller (apply.save_results) then has the .npz store, and says so - nothing is written silently in another format.

Files written here open with ``h5py.File(path)`` / ``h5dump``; files written by the reference's loop (h5py defaults: contiguous
little-endian float32) read back with H5Store(path).  Not covered: filtered datasets (the reference's INPUT stores use h5py's own
"lzf" filter, src/dataset.py:63 - a plugin the C library does not ship), compound types.

The dataset layout of the reference's build (processing/build_dataset.py, written with h5py) needs a little more, added below the store's
result-file interface without changing it: groups, attributes on groups and datasets (H5Store.create_group / set_attrs / attrs), datasets
written with create_dataset (optional deflate, h5py's compression="gzip") and read with read(): fixed-length NULLPAD ASCII strings (what
h5py writes for np.string_ arrays) and numpy bool stored as h5py stores it, an 8-bit enum FALSE = 0 / TRUE = 1 that h5py reads back as bool.
"""
import ctypes
import ctypes.util
import glob
import os

import numpy as np

hid_t = ctypes.c_int64
hsize_t = ctypes.c_uint64
herr_t = ctypes.c_int

H5F_ACC_RDONLY, H5F_ACC_TRUNC = 0, 2
H5P_DEFAULT, H5S_ALL = 0, 0
H5_INDEX_NAME, H5_ITER_NATIVE = 0, 2
H5T_INTEGER, H5T_FLOAT, H5T_STRING, H5T_ENUM = 0, 1, 3, 8
H5T_STR_NULLPAD, H5T_CSET_ASCII = 1, 0
H5_ITER_INC = 0
H5T_ORDER_LE = 0
H5T_SGN_NONE = 0


class H5Unavailable(RuntimeError):
    pass


class H5Error(RuntimeError):
    pass


_lib = None


def _candidates():
    env = os.environ.get("PESTO_HDF5_LIB")
    if env:
        yield env
        return                          # an explicit choice is not second-guessed
    found = ctypes.util.find_library("hdf5") or ctypes.util.find_library("hdf5_serial")
    if found:
        yield found
    for prefix in ("/opt/conda/lib", "/usr/lib/x86_64-linux-gnu", "/usr/lib/x86_64-linux-gnu/hdf5/serial", "/usr/local/lib", "/usr/lib64"):
        for name in ("libhdf5.so", "libhdf5_serial.so"):
            for path in sorted(glob.glob(os.path.join(prefix, name + "*"))):
                yield path


def load():
    """The bound library (cached). Raises H5Unavailable when no HDF5 C library can be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    tried = []
    lib = None
    for path in _candidates():
        try:
            lib = ctypes.CDLL(path)
            break
        except OSError as e:
            tried.append(f"{path}: {e}")
    if lib is None:
        raise H5Unavailable("no HDF5 C library could be loaded (set PESTO_HDF5_LIB to a libhdf5.so); tried: " + ("; ".join(tried) or "nothing found"))
    sig = {
        "H5open": (herr_t, []),
        "H5get_libversion": (herr_t, [ctypes.POINTER(ctypes.c_uint)] * 3),
        "H5Eset_auto2": (herr_t, [hid_t, ctypes.c_void_p, ctypes.c_void_p]),
        "H5Fcreate": (hid_t, [ctypes.c_char_p, ctypes.c_uint, hid_t, hid_t]),
        "H5Fopen": (hid_t, [ctypes.c_char_p, ctypes.c_uint, hid_t]),
        "H5Fflush": (herr_t, [hid_t, ctypes.c_int]),
        "H5Fclose": (herr_t, [hid_t]),
        "H5Pcreate": (hid_t, [hid_t]),
        "H5Pset_create_intermediate_group": (herr_t, [hid_t, ctypes.c_uint]),
        "H5Pclose": (herr_t, [hid_t]),
        "H5Screate_simple": (hid_t, [ctypes.c_int, ctypes.POINTER(hsize_t), ctypes.POINTER(hsize_t)]),
        "H5Sget_simple_extent_ndims": (ctypes.c_int, [hid_t]),
        "H5Sget_simple_extent_dims": (ctypes.c_int, [hid_t, ctypes.POINTER(hsize_t), ctypes.POINTER(hsize_t)]),
        "H5Sclose": (herr_t, [hid_t]),
        "H5Dcreate2": (hid_t, [hid_t, ctypes.c_char_p, hid_t, hid_t, hid_t, hid_t, hid_t]),
        "H5Dopen2": (hid_t, [hid_t, ctypes.c_char_p, hid_t]),
        "H5Dwrite": (herr_t, [hid_t, hid_t, hid_t, hid_t, hid_t, ctypes.c_void_p]),
        "H5Dread": (herr_t, [hid_t, hid_t, hid_t, hid_t, hid_t, ctypes.c_void_p]),
        "H5Dget_space": (hid_t, [hid_t]),
        "H5Dget_type": (hid_t, [hid_t]),
        "H5Dclose": (herr_t, [hid_t]),
        "H5Tget_class": (ctypes.c_int, [hid_t]),
        "H5Tget_size": (ctypes.c_size_t, [hid_t]),
        "H5Tget_sign": (ctypes.c_int, [hid_t]),
        "H5Tclose": (herr_t, [hid_t]),
        "H5Lexists": (ctypes.c_int, [hid_t, ctypes.c_char_p, hid_t]),
        "H5Ldelete": (herr_t, [hid_t, ctypes.c_char_p, hid_t]),
        # groups, attributes, strings, enums, filters (the dataset layout)
        "H5Gcreate2": (hid_t, [hid_t, ctypes.c_char_p, hid_t, hid_t, hid_t]),
        "H5Gclose": (herr_t, [hid_t]),
        "H5Oopen": (hid_t, [hid_t, ctypes.c_char_p, hid_t]),
        "H5Oclose": (herr_t, [hid_t]),
        "H5Acreate2": (hid_t, [hid_t, ctypes.c_char_p, hid_t, hid_t, hid_t, hid_t]),
        "H5Aopen": (hid_t, [hid_t, ctypes.c_char_p, hid_t]),
        "H5Awrite": (herr_t, [hid_t, hid_t, ctypes.c_void_p]),
        "H5Aread": (herr_t, [hid_t, hid_t, ctypes.c_void_p]),
        "H5Aget_space": (hid_t, [hid_t]),
        "H5Aget_type": (hid_t, [hid_t]),
        "H5Aclose": (herr_t, [hid_t]),
        "H5Aiterate2": (herr_t, [hid_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(hsize_t), ctypes.c_void_p, ctypes.c_void_p]),
        "H5Tcopy": (hid_t, [hid_t]),
        "H5Tset_size": (herr_t, [hid_t, ctypes.c_size_t]),
        "H5Tset_strpad": (herr_t, [hid_t, ctypes.c_int]),
        "H5Tset_cset": (herr_t, [hid_t, ctypes.c_int]),
        "H5Tenum_create": (hid_t, [hid_t]),
        "H5Tenum_insert": (herr_t, [hid_t, ctypes.c_char_p, ctypes.c_void_p]),
        "H5Tget_super": (hid_t, [hid_t]),
        "H5Tget_nmembers": (ctypes.c_int, [hid_t]),
        "H5Pset_chunk": (herr_t, [hid_t, ctypes.c_int, ctypes.POINTER(hsize_t)]),
        "H5Pset_deflate": (herr_t, [hid_t, ctypes.c_uint]),
        "H5Zfilter_avail": (ctypes.c_int, [ctypes.c_int]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise H5Unavailable(f"{lib._name} does not export {name}: not an HDF5 >= 1.10 C library")
        fn.restype, fn.argtypes = res, args
    if lib.H5open() < 0:
        raise H5Unavailable(f"H5open failed in {lib._name}")
    lib.H5Eset_auto2(0, None, None)          # errors come back as negative return values -> H5Error here, not a stack dump on stderr
    _lib = lib
    return lib


def _link_visitor(lib):
    """The library's link visitor: H5Lvisit (an exported symbol up to 1.10), H5Lvisit2 or H5Lvisit1 (1.12+, where H5Lvisit is a macro).
    The three differ in the info struct handed to the callback, which the callback here ignores. Resolved on first use (keys())."""
    for name in ("H5Lvisit", "H5Lvisit2", "H5Lvisit1"):
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = herr_t, [hid_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
            return fn
    raise H5Unavailable(f"{lib._name} exports none of H5Lvisit / H5Lvisit2 / H5Lvisit1: the keys of a store cannot be listed")


def available():
    try:
        load()
        return True
    except H5Unavailable:
        return False


def library_version():
    a, b, c = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_uint()
    load().H5get_libversion(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return (a.value, b.value, c.value)


def _gid(name):
    """Value of one of the library's global identifiers (H5T_NATIVE_*_g, H5P_CLS_*_ID_g; valid after H5open)."""
    return hid_t.in_dll(load(), name).value


_NATIVE = {
    np.dtype(np.float32): "H5T_NATIVE_FLOAT_g", np.dtype(np.float64): "H5T_NATIVE_DOUBLE_g",
    np.dtype(np.int8): "H5T_NATIVE_INT8_g", np.dtype(np.uint8): "H5T_NATIVE_UINT8_g",
    np.dtype(np.int16): "H5T_NATIVE_INT16_g", np.dtype(np.uint16): "H5T_NATIVE_UINT16_g",
    np.dtype(np.int32): "H5T_NATIVE_INT32_g", np.dtype(np.uint32): "H5T_NATIVE_UINT32_g",
    np.dtype(np.int64): "H5T_NATIVE_INT64_g", np.dtype(np.uint64): "H5T_NATIVE_UINT64_g",
}


def _check(rc, what):
    if rc < 0:
        raise H5Error(f"HDF5: {what} failed")
    return rc


class H5Store:
    """``with H5Store(path, "w") as hf: hf[key] = array`` / ``H5Store(path)[key]`` / ``.keys()`` - the part of h5py.File the
    reference's result loop uses (interfaceome/apply_model.py:53, :76). Mode "w" truncates, "r" (default) opens read-only."""

    def __init__(self, path, mode="r"):
        lib = load()
        self._lib = lib
        self._id = -1
        self.path = os.fspath(path)
        self.mode = mode
        if mode == "w":
            self._id = lib.H5Fcreate(self.path.encode(), H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT)
        elif mode == "r":
            self._id = lib.H5Fopen(self.path.encode(), H5F_ACC_RDONLY, H5P_DEFAULT)
        else:
            raise ValueError("mode must be 'r' or 'w'")
        if self._id < 0:
            raise H5Error(f"HDF5: cannot {'create' if mode == 'w' else 'open'} {self.path}")
        self._lcpl = -1
        if mode == "w":
            self._lcpl = _check(lib.H5Pcreate(_gid("H5P_CLS_LINK_CREATE_ID_g")), "H5Pcreate(link creation)")
            _check(lib.H5Pset_create_intermediate_group(self._lcpl, 1), "H5Pset_create_intermediate_group")

    # ---- writing
    def __setitem__(self, key, value):
        if self.mode != "w":
            raise H5Error("store is read-only")
        a = np.ascontiguousarray(value)
        if a.dtype == np.bool_:
            a = a.astype(np.uint8)
        if a.dtype not in _NATIVE:
            raise TypeError(f"dtype {a.dtype} has no HDF5 mapping here (float32/64 and the 8..64-bit integers do)")
        lib, name = self._lib, self._name(key)
        if lib.H5Lexists(self._id, name, H5P_DEFAULT) > 0:
            raise H5Error(f"HDF5: name already exists: {key}")          # h5py: "Unable to create dataset (name already exists)"
        dims = (hsize_t * max(a.ndim, 1))(*a.shape)
        space = _check(lib.H5Screate_simple(a.ndim, dims if a.ndim else None, None), "H5Screate_simple")
        try:
            tid = _gid(_NATIVE[a.dtype])
            ds = _check(lib.H5Dcreate2(self._id, name, tid, space, self._lcpl, H5P_DEFAULT, H5P_DEFAULT), f"H5Dcreate2({key})")
            try:
                if a.size:
                    _check(lib.H5Dwrite(ds, tid, H5S_ALL, H5S_ALL, H5P_DEFAULT, a.ctypes.data_as(ctypes.c_void_p)), f"H5Dwrite({key})")
            finally:
                lib.H5Dclose(ds)
        finally:
            lib.H5Sclose(space)

    # ---- reading
    def __getitem__(self, key):
        lib = self._lib
        ds = lib.H5Dopen2(self._id, self._name(key), H5P_DEFAULT)
        if ds < 0:
            raise KeyError(key)
        try:
            space = _check(lib.H5Dget_space(ds), "H5Dget_space")
            try:
                nd = _check(lib.H5Sget_simple_extent_ndims(space), "H5Sget_simple_extent_ndims")
                dims = (hsize_t * max(nd, 1))()
                if nd:
                    _check(lib.H5Sget_simple_extent_dims(space, dims, None), "H5Sget_simple_extent_dims")
                shape = tuple(int(dims[i]) for i in range(nd))
            finally:
                lib.H5Sclose(space)
            ft = _check(lib.H5Dget_type(ds), "H5Dget_type")
            try:
                cls, size = lib.H5Tget_class(ft), int(lib.H5Tget_size(ft))
                if cls == H5T_FLOAT and size in (4, 8):
                    dt = np.dtype(np.float32 if size == 4 else np.float64)
                elif cls == H5T_FLOAT and size == 2:
                    dt = np.dtype(np.float32)                  # half-precision files are widened by the library
                elif cls == H5T_INTEGER and size in (1, 2, 4, 8):
                    dt = np.dtype(("u" if lib.H5Tget_sign(ft) == H5T_SGN_NONE else "i") + str(size))
                else:
                    raise H5Error(f"HDF5: dataset {key}: type class {cls} of {size} bytes is not read here")
            finally:
                lib.H5Tclose(ft)
            out = np.empty(shape, dt)
            if out.size:          # memory type = the native type of `dt`: the library converts byte order / width
                _check(lib.H5Dread(ds, _gid(_NATIVE[dt]), H5S_ALL, H5S_ALL, H5P_DEFAULT, out.ctypes.data_as(ctypes.c_void_p)), f"H5Dread({key})")
            return out
        finally:
            lib.H5Dclose(ds)

    def __contains__(self, key):
        lib = self._lib
        # H5Lexists wants every intermediate link to exist: walk the path
        parts = [p for p in str(key).split("/") if p]
        for i in range(1, len(parts) + 1):
            if lib.H5Lexists(self._id, "/".join(parts[:i]).encode(), H5P_DEFAULT) <= 0:
                return False
        return bool(parts)

    def keys(self):
        """Full names of all DATASETS in the file, in name order (h5py's File.visit order), without the leading '/'."""
        lib, names = self._lib, []
        cb_t = ctypes.CFUNCTYPE(herr_t, hid_t, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p)

        def visit(_group, name, _info, _data):
            names.append(name.decode())
            return 0

        cb = cb_t(visit)
        _check(_link_visitor(lib)(self._id, H5_INDEX_NAME, H5_ITER_NATIVE, ctypes.cast(cb, ctypes.c_void_p), None), "H5Lvisit")
        out = []
        for n in names:                        # links to groups are visited too: keep what opens as a dataset
            ds = lib.H5Dopen2(self._id, n.encode(), H5P_DEFAULT)
            if ds >= 0:
                lib.H5Dclose(ds)
                out.append(n)
        return sorted(out)

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    @staticmethod
    def _name(key):
        name = str(key)
        if not name.strip("/"):
            raise KeyError(key)
        return name.encode()

    # ---- the dataset layout: groups, attributes, strings, bool, deflate
    def create_group(self, path):
        """Create the group ``path`` and any missing parents (h5py's File.create_group; an existing group is an error there too)."""
        if self.mode != "w":
            raise H5Error("store is read-only")
        g = self._lib.H5Gcreate2(self._id, self._name(path), self._lcpl, H5P_DEFAULT, H5P_DEFAULT)
        if g < 0:
            raise H5Error(f"HDF5: cannot create group {path}")
        self._lib.H5Gclose(g)

    def create_dataset(self, name, data, compression=None, attrs=None):
        """h5py's create_dataset(name, data=...) for numeric, bool (8-bit enum FALSE / TRUE) and fixed-length bytes ('S<n>': NULLPAD
        ASCII strings) arrays. compression: None (contiguous) or "gzip" (deflate level 4 in one chunk; H5Unavailable when the library
        has no deflate filter). attrs: {name: value} written on the dataset (set_attrs)."""
        if self.mode != "w":
            raise H5Error("store is read-only")
        if compression not in (None, "gzip"):
            raise ValueError(f"compression must be None or 'gzip', got {compression!r}")
        a = np.ascontiguousarray(data)
        lib = self._lib
        tid, own = _file_type(a)
        dims = (hsize_t * max(a.ndim, 1))(*a.shape)
        space = _check(lib.H5Screate_simple(a.ndim, dims if a.ndim else None, None), "H5Screate_simple")
        dcpl = H5P_DEFAULT
        try:
            if compression and a.ndim and a.size:
                if lib.H5Zfilter_avail(1) <= 0:                           # H5Z_FILTER_DEFLATE
                    raise H5Unavailable("this HDF5 C library has no deflate filter")
                dcpl = _check(lib.H5Pcreate(_gid("H5P_CLS_DATASET_CREATE_ID_g")), "H5Pcreate(dataset creation)")
                _check(lib.H5Pset_chunk(dcpl, a.ndim, dims), "H5Pset_chunk")
                _check(lib.H5Pset_deflate(dcpl, 4), "H5Pset_deflate")
            ds = _check(lib.H5Dcreate2(self._id, self._name(name), tid, space, self._lcpl, dcpl, H5P_DEFAULT), f"H5Dcreate2({name})")
            try:
                if a.size:
                    _check(lib.H5Dwrite(ds, tid, H5S_ALL, H5S_ALL, H5P_DEFAULT, a.ctypes.data_as(ctypes.c_void_p)), f"H5Dwrite({name})")
            finally:
                lib.H5Dclose(ds)
        finally:
            if dcpl != H5P_DEFAULT:
                lib.H5Pclose(dcpl)
            lib.H5Sclose(space)
            if own:
                lib.H5Tclose(tid)
        if attrs:
            self.set_attrs(name, attrs)

    def set_attrs(self, path, attrs):
        """Write {name: value} as attributes of the group or dataset ``path`` (h5py's obj.attrs[name] = value): numbers and tuples of
        ints as arrays (int64 for Python ints, as h5py stores a shape), numpy arrays as they are, bool arrays as the 8-bit enum."""
        if self.mode != "w":
            raise H5Error("store is read-only")
        lib = self._lib
        obj = _check(lib.H5Oopen(self._id, self._name(path), H5P_DEFAULT), f"H5Oopen({path})")
        try:
            for k, v in attrs.items():
                a = np.ascontiguousarray(np.asarray(v, dtype=np.int64) if isinstance(v, (tuple, list, int)) and not isinstance(v, bool)
                                         else np.asarray(v))
                tid, own = _file_type(a)
                dims = (hsize_t * max(a.ndim, 1))(*a.shape)
                space = _check(lib.H5Screate_simple(a.ndim, dims if a.ndim else None, None), "H5Screate_simple")
                try:
                    at = _check(lib.H5Acreate2(obj, str(k).encode(), tid, space, H5P_DEFAULT, H5P_DEFAULT), f"H5Acreate2({path}:{k})")
                    try:
                        if a.size:
                            _check(lib.H5Awrite(at, tid, a.ctypes.data_as(ctypes.c_void_p)), f"H5Awrite({path}:{k})")
                    finally:
                        lib.H5Aclose(at)
                finally:
                    lib.H5Sclose(space)
                    if own:
                        lib.H5Tclose(tid)
        finally:
            lib.H5Oclose(obj)

    def attrs(self, path):
        """{name: numpy value} of the attributes of the group or dataset ``path``, in name order (the 8-bit enum as bool)."""
        lib = self._lib
        obj = lib.H5Oopen(self._id, self._name(path), H5P_DEFAULT)
        if obj < 0:
            raise KeyError(path)
        names = []
        cb_t = ctypes.CFUNCTYPE(herr_t, hid_t, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p)

        def visit(_loc, name, _info, _data):
            names.append(name.decode())
            return 0

        try:
            cb = cb_t(visit)
            _check(lib.H5Aiterate2(obj, H5_INDEX_NAME, H5_ITER_INC, None, ctypes.cast(cb, ctypes.c_void_p), None), "H5Aiterate2")
            out = {}
            for n in names:
                at = _check(lib.H5Aopen(obj, n.encode(), H5P_DEFAULT), f"H5Aopen({n})")
                try:
                    out[n] = _read_object(lib, at, lib.H5Aget_space, lib.H5Aget_type, lambda mt, buf: lib.H5Aread(at, mt, buf), n)
                finally:
                    lib.H5Aclose(at)
            return out
        finally:
            lib.H5Oclose(obj)

    def read(self, key):
        """The dataset ``key`` as numpy: what __getitem__ reads, plus fixed-length strings (bytes, 'S<n>') and the 8-bit bool enum (bool)."""
        lib = self._lib
        ds = lib.H5Dopen2(self._id, self._name(key), H5P_DEFAULT)
        if ds < 0:
            raise KeyError(key)
        try:
            return _read_object(lib, ds, lib.H5Dget_space, lib.H5Dget_type,
                                lambda mt, buf: lib.H5Dread(ds, mt, H5S_ALL, H5S_ALL, H5P_DEFAULT, buf), key)
        finally:
            lib.H5Dclose(ds)

    # ---- life cycle
    def flush(self):
        if self._id >= 0:
            _check(self._lib.H5Fflush(self._id, 1), "H5Fflush")          # scope 1 = H5F_SCOPE_GLOBAL

    def close(self):
        if self._id >= 0:
            if self._lcpl >= 0:
                self._lib.H5Pclose(self._lcpl)
                self._lcpl = -1
            rc = self._lib.H5Fclose(self._id)
            self._id = -1
            _check(rc, f"H5Fclose({self.path})")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bool_type():
    """h5py's bool: an enum over a signed 8-bit integer, FALSE = 0, TRUE = 1 (a new type id; the caller closes it)."""
    lib = load()
    t = _check(lib.H5Tenum_create(_gid("H5T_NATIVE_INT8_g")), "H5Tenum_create")
    for name, v in ((b"FALSE", 0), (b"TRUE", 1)):
        c = ctypes.c_int8(v)
        _check(lib.H5Tenum_insert(t, name, ctypes.byref(c)), "H5Tenum_insert")
    return t


def _file_type(a):
    """(type id, owned) for the elements of numpy array ``a``: the native numeric types, the bool enum, fixed-length NULLPAD ASCII."""
    lib = load()
    if a.dtype == np.bool_:
        return _bool_type(), True
    if a.dtype.kind == "S":
        t = _check(lib.H5Tcopy(_gid("H5T_C_S1_g")), "H5Tcopy")
        _check(lib.H5Tset_size(t, max(1, a.dtype.itemsize)), "H5Tset_size")
        _check(lib.H5Tset_strpad(t, H5T_STR_NULLPAD), "H5Tset_strpad")
        _check(lib.H5Tset_cset(t, H5T_CSET_ASCII), "H5Tset_cset")
        return t, True
    if a.dtype not in _NATIVE:
        raise TypeError(f"dtype {a.dtype} has no HDF5 mapping here (numbers, bool and fixed-length bytes do)")
    return _gid(_NATIVE[a.dtype]), False


def _read_object(lib, obj, get_space, get_type, read, what):
    """Read a dataset or attribute: numbers (native), fixed-length strings (bytes) and 8-bit enums of FALSE / TRUE (bool)."""
    space = _check(get_space(obj), "get_space")
    try:
        nd = _check(lib.H5Sget_simple_extent_ndims(space), "H5Sget_simple_extent_ndims")
        dims = (hsize_t * max(nd, 1))()
        if nd:
            _check(lib.H5Sget_simple_extent_dims(space, dims, None), "H5Sget_simple_extent_dims")
        shape = tuple(int(dims[i]) for i in range(nd))
    finally:
        lib.H5Sclose(space)
    ft = _check(get_type(obj), "get_type")
    mt, own, post = None, False, None
    try:
        cls, size = lib.H5Tget_class(ft), int(lib.H5Tget_size(ft))
        if cls == H5T_FLOAT and size in (4, 8):
            dt = np.dtype(np.float32 if size == 4 else np.float64)
        elif cls == H5T_INTEGER and size in (1, 2, 4, 8):
            dt = np.dtype(("u" if lib.H5Tget_sign(ft) == H5T_SGN_NONE else "i") + str(size))
        elif cls == H5T_STRING:
            dt = np.dtype(f"S{size}")
            mt = _check(lib.H5Tcopy(ft), "H5Tcopy")           # the file's own string type: the library copies the bytes as they are
            own = True
        elif cls == H5T_ENUM and size == 1:
            dt, mt, own, post = np.dtype(np.int8), _bool_type(), True, (lambda v: v.astype(bool))
        else:
            raise H5Error(f"HDF5: {what}: type class {cls} of {size} bytes is not read here")
        out = np.empty(shape, dt)
        if out.size:
            _check(read(mt if mt is not None else _gid(_NATIVE[dt]), out.ctypes.data_as(ctypes.c_void_p)), f"read({what})")
        return post(out) if post else out
    finally:
        if own:
            lib.H5Tclose(mt)
        lib.H5Tclose(ft)
