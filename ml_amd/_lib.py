"""ctypes binding of the C ABI (include/mlhip.h). Loads ml_amd/libmlhip.so; never falls back to anything else."""
import ctypes as C
import os
import re
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MLHIP_LIBRARY") or os.path.join(_HERE, "libmlhip.so")   # override: sanitizer / debug builds

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(or `make -C ml_amd/csrc`). ml_amd has no CPU fallback.")



def _preload_shared_hip_runtime():
    """A process must run ONE HIP runtime. PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 with the
    same sonames as /opt/rocm's, and the dynamic loader keeps whichever copy is loaded first: if this library pulled in
    the system copy first, a later `import torch` would bind to a runtime it was not built against and report no GPU.
    So when a torch installation is present (it is only ever used for torch.distributed collectives), load its
    runtime libraries first -- without importing torch. MLHIP_HIP_RUNTIME=system opts out."""
    if os.environ.get("MLHIP_HIP_RUNTIME", "").lower() == "system":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            path = os.path.join(libdir, name)
            if os.path.exists(path):
                C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError:
        pass   # fall back to the system runtime named in libmlhip.so's DT_NEEDED


_preload_shared_hip_runtime()
lib = C.CDLL(LIB_PATH)

OK, E_INVALID_ARGUMENT, E_DOMAIN, E_RUNTIME, E_NO_DEVICE, E_UNSUPPORTED = 0, -1, -2, -3, -4, -5

c_dp = C.POINTER(C.c_double)
c_u32p = C.POINTER(C.c_uint32)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)

DEFAULT_COVARIANCE_RIDGE = 1e-15      # MLHIP_DEFAULT_COVARIANCE_RIDGE


class EmRouteInfo(C.Structure):
    """mlhip_em_route_info"""
    _fields_ = [(name, C.c_int32) for name in ("estep", "fused", "fused_form", "self_norm", "sparse", "balanced", "fold_allowed",
                                               "diag_kernel", "diag_exact", "device_close", "records_on_device", "resident")]


class KmeansRouteInfo(C.Structure):
    """mlhip_kmeans_route_info"""
    _fields_ = [(name, C.c_int32) for name in ("kernel", "pad", "resident")]


# ---- prototypes: read from the headers, so that every call converts its arguments as the C declaration says ----------------
_SCALARS = {"int": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "size_t": C.c_size_t,
            "double": C.c_double}
_OPAQUE = ("void", "mlhip_ctx", "mlhip_data", "mlpp_em", "mlpp_kmeans", "mlpp_centroids_initialiser", "mlpp_responsibilities_initialiser")
_STRUCTS = {"mlhip_em_route_info": EmRouteInfo, "mlhip_kmeans_route_info": KmeansRouteInfo}
_RETURNS = {"int": C.c_int, "const char*": C.c_char_p}


def _ctype(spelling):
    """The ctypes type of a parameter type as the headers spell it ('const double*', 'uint64_t[4]'); None outside their vocabulary."""
    if spelling in ("const char*", "const char**"):
        return C.c_char_p if spelling.endswith("r*") else C.POINTER(C.c_char_p)
    base = re.sub(r"\[\d+\]$", "*", spelling.replace("const ", "").replace("struct ", ""))
    base, stars = base.rstrip("*"), len(base) - len(base.rstrip("*"))
    if base in _SCALARS and stars <= 1:
        return C.POINTER(_SCALARS[base]) if stars else _SCALARS[base]
    if base in _OPAQUE and 1 <= stars <= 2:
        return C.c_void_p
    if base in _STRUCTS and stars == 1:
        return C.POINTER(_STRUCTS[base])
    return ALLREDUCE_FN if spelling == "mlhip_allreduce_fn" else None


def _prototypes(text):
    """{function: (restype, argtypes)} for every function a header's text declares. ImportError for a type outside the table above:
    no declaration is passed over, so no function goes without a prototype."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)                                    # comments
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)                               # preprocessor lines
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;|typedef[^;{]*;", "", text, flags=re.S)   # the structs, the hook's type
    found = {}
    for returns, name, parameters in re.findall(r"([\w \t*]+?)\s*\b(ml(?:hip|pp)_\w+)\s*\(([^()]*)\)\s*;", text):
        spellings = [returns] + ([] if parameters.strip() == "void" else parameters.split(","))
        spellings = [re.sub(r"\s*\*", "*", " ".join(s.split())) for s in spellings]
        spellings[1:] = [re.sub(r"\s*\b\w+(\[\d+\])?$", r"\1", s) for s in spellings[1:]]   # without the parameter's name
        types = [_RETURNS.get(spellings[0])] + [_ctype(s) for s in spellings[1:]]
        if None in types:
            raise ImportError(f"{name}: no ctypes type for '{spellings[types.index(None)]}' (ml_amd/_lib.py, _ctype)")
        found[name] = (types[0], types[1:])
    return found


for _header in ("mlhip.h", "mlpp_c.h"):
    with open(os.path.join(os.path.dirname(_HERE), "include", _header)) as _f:
        for _name, (_restype, _argtypes) in _prototypes(_f.read()).items():
            getattr(lib, _name).restype, getattr(lib, _name).argtypes = _restype, _argtypes


class MlhipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class NoDeviceError(MlhipError):
    pass


def check(rc):
    if rc == OK:
        return
    msg = lib.mlhip_last_error().decode()
    if rc in (E_INVALID_ARGUMENT, E_DOMAIN):
        raise ValueError(msg)          # pybind11 maps invalid_argument / domain_error to ValueError
    if rc == E_NO_DEVICE:
        raise NoDeviceError(rc, msg)
    raise MlhipError(rc, msg)


def dptr(a):
    """The array's memory as double* (None, an output not asked for, stays None: NULL)."""
    return None if a is None else a.ctypes.data_as(c_dp)


def u32ptr(a):
    return None if a is None else a.ctypes.data_as(c_u32p)


def _float64_copy(a, dtype=np.float64):
    return np.array(a, dtype=dtype, order="C")


def _float64(a, copy=False):
    return _float64_copy(a) if copy else np.ascontiguousarray(a, np.float64)


def _shape_error(name, a, shape):
    return ValueError(f"{name} has shape {a.shape}, expected {shape}")


def _require_shape(name, a, *shape):
    if a.shape != shape:
        raise _shape_error(name, a, shape)


def _is_block(x):
    """What every call that takes rows of data accepts as they are: a C-contiguous float64 N x d numpy array, never converted."""
    return isinstance(x, np.ndarray) and x.dtype == np.float64 and x.ndim == 2 and x.flags.c_contiguous


def _covariance_shape(K, d, diagonal, tied):
    if diagonal and tied:
        raise ValueError("diagonal and tied exclude each other")
    return (d, d) if tied else (K, d) if diagonal else (K, d, d)


def mixture_arguments(mixing, means, covs, diagonal=False, tied=False, d=None, copy=False, restarts=False):
    """The parameters of a mixture as the library takes them, checked before any call: (K, d, covariance_type, mixing, means, covs),
    the arrays C-contiguous float64 (copy=True: fresh copies, for the calls that update them in place), covariance_type 0 full /
    1 diagonal / 2 tied. mixing: K (None for a call that takes none: K is then the number of rows of means); means: K x d; covs:
    K x d x d, K x d with diagonal=True, d x d with tied=True; restarts=True: each under one leading axis R. d: the dimension they
    must have (a block's). ValueError names the array, its shape and the shape expected."""
    convert = _float64_copy if copy else np.ascontiguousarray           # (kept lean: this runs before every step call)
    means, covs = convert(means, np.float64), convert(covs, np.float64)
    if mixing is None:
        head = means.shape[:-1]
    else:
        mixing = convert(mixing, np.float64)
        head = mixing.shape                                             # (K,), or (R, K) with restarts
    if len(head) != (2 if restarts else 1):
        lead = "(R, K" if restarts else "(K"
        raise ValueError(f"means has shape {means.shape}, expected {lead}, d)" if mixing is None else
                         f"mixing has shape {head}, expected {lead}{')' if restarts else ',)'}")
    K = head[-1]
    if d is None:
        d = means.shape[-1] if means.ndim else 0
    if means.shape != head + (d,):
        raise _shape_error("means", means, head + (d,))
    expected = head[:-1] + _covariance_shape(K, d, diagonal, tied)
    if covs.shape != expected:
        raise _shape_error("covs", covs, expected)
    return K, d, 2 if tied else 1 if diagonal else 0, mixing, means, covs


def conditioned_arguments(d_observed, mixing, means_observed, covs_observed, maps, means_missing, **extra):
    """A conditioned mixture (what em_condition returns) as the five conditioning calls take it, checked before any call: (K, dM,
    arrays), arrays the five and then `extra` in the order given, C-contiguous float64. d_observed: the dimension of the block of
    observed coordinates. extra: factors, covs_missing (K x dM x dM), scales, inverse_scales (K x dM). ValueError names the array,
    its shape and the shape expected."""
    arrays = {name: _float64(a) for name, a in dict(mixing=mixing, means_observed=means_observed, covs_observed=covs_observed, maps=maps,
                                                    means_missing=means_missing, **extra).items()}
    if arrays["means_missing"].ndim != 2:
        raise ValueError(f"means_missing has shape {arrays['means_missing'].shape}, expected (K, dM)")
    K, dM = arrays["means_missing"].shape
    shapes = dict(mixing=(K,), means_observed=(K, d_observed), covs_observed=(K, d_observed, d_observed), maps=(K, dM, d_observed),
                  means_missing=(K, dM), factors=(K, dM, dM), covs_missing=(K, dM, dM), scales=(K, dM), inverse_scales=(K, dM))
    if set(extra) - set(shapes):
        raise TypeError(f"conditioned_arguments() got an unexpected keyword argument {sorted(set(extra) - set(shapes))[0]!r}")
    for name, a in arrays.items():
        _require_shape(name, a, *shapes[name])
    return K, dM, list(arrays.values())


def _route_name(fn, names, *args, after=()):
    """The name of the route a `*_route` entry point reports: fn(*args, &route, *after)."""
    route = C.c_int()
    check(fn(*args, C.byref(route), *after))
    return names[route.value]


def _with_optional(out, *optional):
    """`out`, or the tuple of it and the optional outputs that were asked for (not None), in the order given."""
    extra = [v for v in optional if v is not None]
    return (out, *extra) if extra else out


def _get(fn, handle, ctype):
    """A scalar the library returns through an out-pointer: fn(handle, &value)."""
    v = ctype()
    check(fn(handle, C.byref(v)))
    return v.value


def em_select_restart(log_likelihood, converged):
    """The restart mlhip_em_iterate_restarts keeps (mlhip_em_select_restart; no GPU needed): the greatest log-likelihood among the
    converged restarts, else among all; strict '>', so the first of equals; a NaN never wins, all NaN gives 0."""
    ll = np.ascontiguousarray(log_likelihood, dtype=np.float64)
    conv = np.ascontiguousarray(converged, dtype=np.int32)
    if ll.ndim != 1:
        raise ValueError(f"log_likelihood has shape {ll.shape}, expected (R,)")
    _require_shape("converged", conv, *ll.shape)
    best = C.c_uint32()
    check(lib.mlhip_em_select_restart(len(ll), dptr(ll), conv.ctypes.data_as(C.POINTER(C.c_int)), C.byref(best)))
    return best.value


RCCL_UNIQUE_ID_BYTES = 128


def rccl_available():
    """Whether librccl can be loaded in this process (no GPU touched): agree on it across ranks BEFORE Context.init_rccl."""
    return bool(lib.mlhip_rccl_available())


def rccl_unique_id():
    """128 opaque bytes from ncclGetUniqueId (rank 0 calls this and hands them to every rank: Context.init_rccl)."""
    buf = C.create_string_buffer(RCCL_UNIQUE_ID_BYTES)
    check(lib.mlhip_rccl_unique_id(buf))
    return buf.raw


def device_count():
    n = C.c_int()
    check(lib.mlhip_device_count(C.byref(n)))
    return n.value


class Context:
    """One GPU + stream (mlhip_ctx) -- or, made by Context.group(...), a device GROUP: one context over several shards (GPUs), to
    which Data uploads row-shard the caller's block and every call fans out (mlhip_ctx_create_group)."""

    def __init__(self, device_id=-1):
        self._fill(C.c_void_p(), True)
        check(lib.mlhip_ctx_create(int(device_id), C.byref(self._h)))

    def _fill(self, handle, owned):
        """The fields of a context, set here and nowhere else (__init__, group, borrow)."""
        self._h = handle
        self._hook = None
        self._owned = owned
        self._blocks = weakref.WeakSet()      # live Data objects: they hold a pointer to this context
        return self

    @classmethod
    def group(cls, n_shards=None, device_ids=None):
        """A device group of n_shards shards, shard s on GPU device_ids[s] (default: s mod the number of GPUs; ids may repeat --
        8 shards on one GPU rehearse the 8-GPU configurations on a one-GPU box)."""
        if device_ids is not None:
            ids = [int(v) for v in device_ids]
            n_shards = len(ids) if n_shards is None else int(n_shards)
            if n_shards != len(ids):
                raise ValueError("device_ids must name one GPU per shard")
            arr = (C.c_int * n_shards)(*ids)
        else:
            n_shards = device_count() if n_shards is None else int(n_shards)
            arr = None
        self = cls.__new__(cls)._fill(C.c_void_p(), True)
        check(lib.mlhip_ctx_create_group(n_shards, arr, C.byref(self._h)))
        return self

    @property
    def shards(self):
        return _get(lib.mlhip_ctx_shards, self._h, C.c_int)

    @property
    def shard_devices(self):
        out = []
        for s in range(self.shards):
            d = C.c_int()
            check(lib.mlhip_ctx_shard_device(self._h, s, C.byref(d)))
            out.append(d.value)
        return out

    @property
    def reduce_kind(self):
        """How the statistics are summed: none / hook-host / hook-device / rccl / group-rccl / group-direct."""
        return _get(lib.mlhip_ctx_reduce_kind, self._h, C.c_char_p).decode()

    @classmethod
    def borrow(cls, handle):
        """Wraps a context owned by someone else (the C++ facade's process-wide one): close() leaves it alive."""
        return cls.__new__(cls)._fill(handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle), False)

    def close(self):
        if getattr(self, "_h", None):
            for block in list(self._blocks):  # a sample block must not outlive its context
                block.close()
            if self._owned:
                lib.mlhip_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def handle(self):
        return self._h

    @property
    def device(self):
        return _get(lib.mlhip_ctx_device, self._h, C.c_int)

    @property
    def stream(self):
        return _get(lib.mlhip_ctx_stream, self._h, C.c_void_p) or 0

    def synchronize(self):
        check(lib.mlhip_ctx_synchronize(self._h))

    def set_allreduce(self, fn, on_device, world_size, rank):
        """fn(ptr:int, count:int, on_device:bool, stream:int) -> None sums the buffer in place across ranks."""
        if fn is None:
            self._hook = None
            check(lib.mlhip_ctx_set_allreduce(self._h, C.cast(None, ALLREDUCE_FN), None, 0, 1, 0))
            return

        def trampoline(_user, buf, count, on_dev, stream):
            try:
                fn(buf or 0, count, bool(on_dev), stream or 0)
                return 0
            except Exception:  # surfaced as MLHIP_E_RUNTIME by the library
                import traceback
                traceback.print_exc()
                return 1

        self._hook = ALLREDUCE_FN(trampoline)
        check(lib.mlhip_ctx_set_allreduce(self._h, self._hook, None, int(on_device), int(world_size), int(rank)))

    def init_rccl(self, unique_id, world_size, rank):
        """The library's own RCCL communicator (collective call): statistics are summed by ncclAllReduce on the context's
        stream, no Python in the iteration."""
        if len(unique_id) != RCCL_UNIQUE_ID_BYTES:
            raise ValueError("unique_id must be the 128 bytes of rccl_unique_id()")
        self._hook = None
        check(lib.mlhip_ctx_init_rccl(self._h, C.c_char_p(bytes(unique_id)), int(world_size), int(rank)))

    def init_rccl_file(self, path, world_size, rank):
        check(lib.mlhip_ctx_init_rccl_file(self._h, os.fsencode(path), int(world_size), int(rank)))

    @property
    def rccl_ranks(self):
        """Ranks of the library-owned communicator as RCCL counts them (0: none)."""
        return _get(lib.mlhip_ctx_rccl_ranks, self._h, C.c_int)

    def finalize_rccl(self):
        check(lib.mlhip_ctx_finalize_rccl(self._h))

    @property
    def world(self):
        w, r = C.c_int(), C.c_int()
        check(lib.mlhip_ctx_world(self._h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def _sample_arguments(self, mixing, means, covs, n, seed, first_row, diagonal, tied):
        K, d, mode, *keep = mixture_arguments(mixing, means, covs, diagonal, tied)
        if n < 0:
            raise ValueError("the number of rows must not be negative")
        return (self._h, d, K, mode, *map(dptr, keep), seed, first_row, n), keep, d

    def em_sample(self, mixing, means, covs, n, seed=0, first_row=0, diagonal=False, tied=False):
        """Rows [first_row, first_row + n) of the sample that `seed` and the mixture define, drawn on the device (mlhip_em_sample):
        (X, labels), X n x d C-contiguous float64, labels uint32. means: K x d; covs: K x d x d (K x d variances with diagonal=True,
        the one d x d matrix with tied=True). A row depends on (seed, its global index) only."""
        args, keep, d = self._sample_arguments(mixing, means, covs, n, seed, first_row, diagonal, tied)
        X, labels = np.empty((n, d)), np.empty(n, dtype=np.uint32)
        check(lib.mlhip_em_sample(*args, dptr(X), d, u32ptr(labels)))
        return X, labels

    def em_sample_data(self, mixing, means, covs, n, seed=0, first_row=0, diagonal=False, tied=False):
        """The same rows as a resident block that never leaves the device (mlhip_em_sample_data): (Data, labels)."""
        args, keep, d = self._sample_arguments(mixing, means, covs, n, seed, first_row, diagonal, tied)
        labels = np.empty(n, dtype=np.uint32)
        handle = C.c_void_p()
        check(lib.mlhip_em_sample_data(*args, u32ptr(labels), C.byref(handle)))
        return Data.adopt(self, handle, n, d), labels

    def timing_enable(self, on=True):
        check(lib.mlhip_timing_enable(self._h, int(on)))

    def timing_reset(self):
        check(lib.mlhip_timing_reset(self._h))

    def timing_get(self, name):
        ms, cnt = C.c_double(), C.c_uint64()
        check(lib.mlhip_timing_get(self._h, name.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value


def require_weights(w, n):
    """Row weights as the library takes them: TypeError unless a float64 numpy array (no conversion, like `fit`'s data),
    ValueError unless 1-D, C-contiguous and of length n. Checked before any device call."""
    if not (isinstance(w, np.ndarray) and w.dtype == np.float64):
        raise TypeError("weights must be a float64 numpy array")
    if w.ndim != 1 or not w.flags.c_contiguous or w.shape[0] != n:
        raise ValueError(f"weights must be a 1-D C-contiguous array with one value per row ({n})")
    return w


class Data:
    """A d x N sample block resident in HBM (mlhip_data). `x` is N x d float64 C-contiguous."""

    def __init__(self, ctx, x=None, device_ptr=None, shape=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        if x is not None:
            if not _is_block(x):
                raise TypeError("data must be a C-contiguous float64 N x d numpy array")
            n, d = x.shape
            check(lib.mlhip_data_upload(ctx.handle, dptr(x), d, n, d, C.byref(self._h)))
        else:
            n, d = shape
            check(lib.mlhip_data_upload_dev(ctx.handle, C.cast(C.c_void_p(device_ptr), c_dp), d, n, d, C.byref(self._h)))
        self.n, self.d = n, d
        ctx._blocks.add(self)

    @classmethod
    def adopt(cls, ctx, handle, n, d):
        """Wraps a block the library made itself (Context.em_sample_data): owned from here on, freed by close() like an upload."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self._h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        self.n, self.d = int(n), int(d)
        ctx._blocks.add(self)
        return self

    def close(self):
        if getattr(self, "_h", None):
            lib.mlhip_data_free(self._h)
            self._h = None
            self.ctx._blocks.discard(self)

    def __del__(self):
        self.close()

    @property
    def handle(self):
        return self._h

    @property
    def n_global(self):
        ng = C.c_uint64()
        check(lib.mlhip_data_shape(self._h, None, None, C.byref(ng)))
        return ng.value

    def shard_rows(self, shard):
        """(first_row, n_rows) of the rows shard `shard` of a device group holds."""
        lo, cnt = C.c_uint64(), C.c_uint64()
        check(lib.mlhip_data_shard_rows(self._h, int(shard), C.byref(lo), C.byref(cnt)))
        return lo.value, cnt.value

    @property
    def shift(self):
        out = np.empty(self.d)
        check(lib.mlhip_data_shift(self._h, dptr(out)))
        return out

    def set_weights(self, w):
        """Frequency weights of the block's rows (mlhip_data_set_weights): a 1-D C-contiguous float64 array of length N, every
        value finite and >= 0, their total positive; None removes them. TypeError for another type or dtype, ValueError for a
        wrong length or refused values (the block is then unweighted). EM entry points are weighted from here on; per-row
        results (responsibilities, labels, em_score), the initialisers and the K-means calls are not -- unless those are called
        with weighted=True."""
        if w is not None:
            w = require_weights(w, self.n)
        check(lib.mlhip_data_set_weights(self.ctx.handle, self._h, dptr(w)))

    @property
    def weight_sum(self):
        """W, the all-reduced total of the attached weights (the row count of an unweighted block)."""
        return _get(lib.mlhip_data_weight_sum, self._h, C.c_double)

    def set_covariance_ridge(self, ridge):
        """The covariance ridge of the handle (mlhip_data_set_covariance_ridge): what every M-step on it adds to the diagonal of each
        covariance it forms. Finite and >= 0; ValueError otherwise (the handle keeps its ridge). E-step results stay valid."""
        check(lib.mlhip_data_set_covariance_ridge(self.ctx.handle, self._h, ridge))

    @property
    def covariance_ridge(self):
        """The handle's covariance ridge (DEFAULT_COVARIANCE_RIDGE = 1e-15 unless set)."""
        return _get(lib.mlhip_data_covariance_ridge, self._h, C.c_double)

    # ---- EM -----------------------------------------------------------------------------------------------
    # Parameter conventions (Python side): means K x d, covariances K x d x d, mixing K.
    def em_step(self, mixing, means, covs):
        K, _, _, mixing, means, covs = mixture_arguments(mixing, means, covs, d=self.d)
        ll = C.c_double()
        pi1, mu1, S1 = np.empty(K), np.empty((K, self.d)), np.empty((K, self.d, self.d))
        check(lib.mlhip_em_step(self.ctx.handle, self._h, K, dptr(mixing), dptr(means), dptr(covs), C.byref(ll),
                                dptr(pi1), dptr(mu1), dptr(S1)))
        return ll.value, pi1, mu1, S1

    def em_step_diag(self, mixing, means, variances):
        """Diagonal-covariance extension. variances: K x d (a K x d x d stack of diagonal matrices is accepted too and
        returned in the same form)."""
        v = np.asarray(variances, dtype=np.float64)
        stacked = v.ndim == 3
        if stacked:
            v = np.stack([np.diag(m) for m in v])
        K, _, _, mixing, means, v = mixture_arguments(mixing, means, v, diagonal=True, d=self.d)
        ll = C.c_double()
        pi1, mu1, v1 = np.empty(K), np.empty((K, self.d)), np.empty((K, self.d))
        check(lib.mlhip_em_step_diag(self.ctx.handle, self._h, K, dptr(mixing), dptr(means), dptr(v), C.byref(ll),
                                     dptr(pi1), dptr(mu1), dptr(v1)))
        if stacked:
            v1 = np.stack([np.diag(row) for row in v1])
        return ll.value, pi1, mu1, v1

    def em_step_tied(self, mixing, means, cov):
        """Tied-covariance extension (mlhip_em_step_tied). cov: the one d x d matrix shared by all components.
        Returns (log_likelihood, mixing, means, cov)."""
        K, _, _, mixing, means, cov = mixture_arguments(mixing, means, cov, tied=True, d=self.d)
        ll = C.c_double()
        pi1, mu1, S1 = np.empty(K), np.empty((K, self.d)), np.empty((self.d, self.d))
        check(lib.mlhip_em_step_tied(self.ctx.handle, self._h, K, dptr(mixing), dptr(means), dptr(cov), C.byref(ll),
                                     dptr(pi1), dptr(mu1), dptr(S1)))
        return ll.value, pi1, mu1, S1

    def em_tied_route(self, K):
        """The route of a tied-covariance step of K components under the switches as they are set now (mlhip_em_tied_route):
        'composed' | 'kernel'."""
        return _route_name(lib.mlhip_em_tied_route, ("composed", "kernel"), self._h, K)

    def em_iterate(self, mixing, means, covs, max_steps, atol=0.0, rtol=0.0, diagonal=False, tied=False):
        """The EM loop in one call (mlhip_em_iterate): up to max_steps iterations with the reference's convergence test, the
        closing arithmetic on the device. covs: K x d x d (or K x d variances with diagonal=True, the one d x d matrix with tied=True).
        Returns (steps_done, converged, log_likelihood, mixing, means, covs, log_likelihood_history)."""
        K, _, mode, pi, mu, S = mixture_arguments(mixing, means, covs, diagonal, tied, d=self.d, copy=True)
        steps, conv, ll = C.c_uint32(), C.c_int(), C.c_double()
        hist = np.full(int(max_steps), np.nan)
        check(lib.mlhip_em_iterate(self.ctx.handle, self._h, K, mode, dptr(pi), dptr(mu), dptr(S), max_steps, atol, rtol,
                                   C.byref(steps), C.byref(conv), C.byref(ll), dptr(hist)))
        return steps.value, bool(conv.value), ll.value, pi, mu, S, hist[:steps.value]

    def em_iterate_restarts(self, mixing, means, covs, max_steps, atol=0.0, rtol=0.0, diagonal=False, tied=False):
        """R EM loops from R starts in one call, and the best of them (mlhip_em_iterate_restarts). mixing: R x K, means: R x K x d,
        covs: R x K x d x d (R x K x d variances with diagonal=True, R x d x d with tied=True). Returns (restarts, best): restarts[r] is
        restart r's tuple, shaped like em_iterate's -- (steps_done, converged, log_likelihood, mixing, means, covs,
        log_likelihood_history) --, best the restart mlhip_em_select_restart picks; em_labels / em_responsibilities afterwards
        are that restart's."""
        K, _, mode, pi, mu, S = mixture_arguments(mixing, means, covs, diagonal, tied, d=self.d, copy=True, restarts=True)
        R = len(pi)
        steps, conv, ll = np.zeros(R, dtype=np.uint32), np.zeros(R, dtype=np.int32), np.full(R, np.nan)
        hist = np.full((R, int(max_steps)), np.nan)
        best = C.c_uint32()
        check(lib.mlhip_em_iterate_restarts(self.ctx.handle, self._h, K, mode, R, dptr(pi), dptr(mu), dptr(S), max_steps, atol, rtol,
                                            u32ptr(steps), conv.ctypes.data_as(C.POINTER(C.c_int)), dptr(ll), dptr(hist), C.byref(best)))
        restarts = [(int(steps[r]), bool(conv[r]), float(ll[r]), pi[r], mu[r], S[r], hist[r, :steps[r]]) for r in range(R)]
        return restarts, best.value

    def em_restarts_route(self, K, R, covariance_type="full"):
        """The route of mlhip_em_iterate_restarts for R restarts of K components under the switches as they are set now
        (mlhip_em_restarts_route): ('sequential' | 'batched', restarts one launch carries)."""
        per_launch = C.c_uint32()
        route = _route_name(lib.mlhip_em_restarts_route, ("sequential", "batched"), self._h, K, {"full": 0, "diag": 1, "tied": 2}[covariance_type], R,
                            after=(C.byref(per_launch),))
        return route, per_launch.value

    def em_plan(self, K):
        """Which kernels a full-covariance EM iteration of K components is made of (mlhip_em_plan):
        {'fused', 'matrix_estep', 'self_norm'} -> bool."""
        f = C.c_uint32()
        check(lib.mlhip_em_plan(self._h, K, C.byref(f)))
        return {"fused": bool(f.value & 1), "matrix_estep": bool(f.value & 2), "self_norm": bool(f.value & 4)}

    def em_screen_counts(self):
        """What the E-step passes of the fits on this block did (mlhip_em_screen_counts): {'screened', 'dense', 'no_information',
        'candidates'} -> int; 'candidates' is the number of pairs the last screened pass evaluated."""
        c = (C.c_uint64 * 4)()
        check(lib.mlhip_em_screen_counts(self.ctx.handle, self._h, c))
        return {"screened": int(c[0]), "dense": int(c[1]), "no_information": int(c[2]), "candidates": int(c[3])}

    def em_route(self, K, covariance_type="full"):
        """The whole route of an EM call of K components under the switches as they are set now (mlhip_em_route): a dict of
        the fields of mlhip_em_route_info, `estep` / `fused_form` by name, the flags as bool, `sparse` as None (by the call
        history), False or True."""
        info = EmRouteInfo()
        check(lib.mlhip_em_route(self._h, K, {"full": 0, "diag": 1}[covariance_type], C.byref(info)))
        out = {name: bool(getattr(info, name)) for name, _ in EmRouteInfo._fields_}
        out["estep"] = ("scalar_fed", "matrix4", "big_dim", "plain")[info.estep]
        out["fused_form"] = ("lds_feed", "scalar_feed", "valu")[info.fused_form] if info.fused else None
        out["sparse"] = None if info.sparse < 0 else bool(info.sparse)
        return out

    def kmeans_route(self, K):
        """The route of a K-means call of K clusters (mlhip_kmeans_route): {'kernel': 'direct' | 'matrix' | 'big_dim' | 'plain',
        'pad': bool, 'resident': bool}."""
        info = KmeansRouteInfo()
        check(lib.mlhip_kmeans_route(self._h, K, C.byref(info)))
        return {"kernel": ("direct", "matrix", "big_dim", "plain")[info.kernel], "pad": bool(info.pad), "resident": bool(info.resident)}

    def em_score(self, mixing, means, covs, diagonal=False, densities=True, labels=True, tied=False):
        """Per-row log-density and label under the given mixture (mlhip_em_score): (log_density, labels), None for the one not
        asked for. covs: K x d x d (or K x d variances with diagonal=True, the one d x d matrix with tied=True). Nothing the handle
        holds is changed."""
        K, _, mode, mixing, means, covs = mixture_arguments(mixing, means, covs, diagonal, tied, d=self.d)
        dens = np.empty(self.n) if densities else None
        lab = np.empty(self.n, dtype=np.uint32) if labels else None
        check(lib.mlhip_em_score(self.ctx.handle, self._h, K, mode, dptr(mixing), dptr(means), dptr(covs), dptr(dens), u32ptr(lab)))
        return dens, lab

    def em_score_route(self, K):
        """The kernel mlhip_em_score runs for K components under the switches as they are set now (mlhip_em_score_route):
        'scalar_fed' | 'matrix4' | 'composed'."""
        return _route_name(lib.mlhip_em_score_route, ("scalar_fed", "matrix4", "composed"), self._h, K)

    def em_conditional_means(self, mixing, means_observed, covs_observed, maps, means_missing, log_density=False):
        """E[x_M | x_O] for every row of this block of OBSERVED coordinates under the conditioned mixture em_condition returns
        (mlhip_em_conditional_means): n x dM C-contiguous float64, and with log_density=True also the n log-densities of the rows
        under the marginal mixture. means_observed: K x dO; covs_observed: K x dO x dO; maps: K x dM x dO; means_missing: K x dM.
        Nothing the handle holds is changed."""
        K, dM, arrays = conditioned_arguments(self.d, mixing, means_observed, covs_observed, maps, means_missing)
        out = np.empty((self.n, dM))
        dens = np.empty(self.n) if log_density else None
        check(lib.mlhip_em_conditional_means(self.ctx.handle, self._h, K, dM, *map(dptr, arrays), dptr(out), dM, dptr(dens)))
        return _with_optional(out, dens)

    def em_condition_route(self, K, dM):
        """The conditioning kernel mlhip_em_conditional_means runs for dM missing coordinates on this block under the switches as they
        are set now (mlhip_em_condition_route): 'registers' | 'plain'."""
        return _route_name(lib.mlhip_em_condition_route, ("registers", "plain"), self._h, K, dM)

    def em_conditional_samples(self, mixing, means_observed, covs_observed, maps, means_missing, factors, n_draws=1, seed=0, first_row=0,
                               first_draw=0, labels=False):
        """Draws from p(x_M | x_O) for every row of this block of OBSERVED coordinates under the conditioned mixture em_condition and
        em_condition_covariances return (mlhip_em_conditional_samples): n_draws x n x dM C-contiguous float64, and with labels=True
        also the n_draws x n components drawn (uint32). factors: K x dM x dM lower Cholesky factors; first_row: the global index of
        the block's row 0; the draws are first_draw .. first_draw + n_draws - 1. Nothing the handle holds is changed."""
        K, dM, arrays = conditioned_arguments(self.d, mixing, means_observed, covs_observed, maps, means_missing, factors=factors)
        if n_draws < 0 or first_draw < 0 or first_draw + n_draws > 2 ** 32 - 1:
            raise ValueError("the draws must lie in 0 .. 2^32 - 2")
        out = np.empty((n_draws, self.n, dM))
        lab = np.empty((n_draws, self.n), dtype=np.uint32) if labels else None
        check(lib.mlhip_em_conditional_samples(self.ctx.handle, self._h, K, dM, *map(dptr, arrays), int(seed), int(first_row),
                                               int(first_draw), int(n_draws), dptr(out), dM, u32ptr(lab)))
        return _with_optional(out, lab)

    def em_conditional_sample_route(self, K, dM):
        """The kernel mlhip_em_conditional_samples runs for dM missing coordinates on this block under the switches as they are set
        now (mlhip_em_conditional_sample_route): 'registers' | 'plain'."""
        return _route_name(lib.mlhip_em_conditional_sample_route, ("registers", "plain"), self._h, K, dM)

    def em_expectation(self, mixing, means, covs):
        K, _, _, mixing, means, covs = mixture_arguments(mixing, means, covs, d=self.d)
        ll = C.c_double()
        check(lib.mlhip_em_expectation(self.ctx.handle, self._h, K, dptr(mixing), dptr(means), dptr(covs), C.byref(ll)))
        return ll.value

    def em_maximisation(self, K):
        pi1, mu1, S1 = np.empty(K), np.empty((K, self.d)), np.empty((K, self.d, self.d))
        check(lib.mlhip_em_maximisation(self.ctx.handle, self._h, K, dptr(pi1), dptr(mu1), dptr(S1)))
        return pi1, mu1, S1

    def em_maximisation_from(self, resp):
        resp = np.asfortranarray(resp, dtype=np.float64)
        if resp.ndim != 2 or len(resp) != self.n:
            raise ValueError(f"resp has shape {resp.shape}, expected one row per row of the block: ({self.n}, K)")
        n, K = resp.shape
        pi1, mu1, S1 = np.empty(K), np.empty((K, self.d)), np.empty((K, self.d, self.d))
        check(lib.mlhip_em_maximisation_from(self.ctx.handle, self._h, K, dptr(resp), n, dptr(pi1), dptr(mu1), dptr(S1)))
        return pi1, mu1, S1

    def em_maximisation_from_labels(self, labels, K):
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        _require_shape("labels", labels, self.n)
        pi1, mu1, S1 = np.empty(K), np.empty((K, self.d)), np.empty((K, self.d, self.d))
        check(lib.mlhip_em_maximisation_from_labels(self.ctx.handle, self._h, K, u32ptr(labels), dptr(pi1), dptr(mu1), dptr(S1)))
        return pi1, mu1, S1

    def em_responsibilities(self, K):
        out = np.empty((self.n, K), order="F")
        check(lib.mlhip_em_responsibilities(self.ctx.handle, self._h, K, dptr(out), self.n))
        return out

    def em_responsibilities_rows(self, K, first, count):
        """Rows [first, first + count) of the responsibilities only (mlhip_em_responsibilities_rows)."""
        out = np.empty((count, K), order="F")
        check(lib.mlhip_em_responsibilities_rows(self.ctx.handle, self._h, K, first, count, dptr(out), max(count, 1)))
        return out

    def em_labels(self, K):
        out = np.empty(self.n, dtype=np.uint32)
        check(lib.mlhip_em_labels(self.ctx.handle, self._h, K, u32ptr(out)))
        return out

    def sample_covariance(self):
        mean, cov = np.empty(self.d), np.empty((self.d, self.d))
        check(lib.mlhip_sample_covariance(self.ctx.handle, self._h, dptr(mean), dptr(cov)))
        return mean, cov

    # ---- K-means --------------------------------------------------------------------------------------------
    def _centroids(self, centroids, copy=False):
        c = _float64(centroids, copy)
        if c.ndim != 2 or c.shape[1] != self.d:
            raise ValueError(f"centroids has shape {c.shape}, expected (K, {self.d})")
        return c

    def kmeans_step(self, centroids, weighted=False):
        """One Lloyd step: (inertia, n_changed, counts, centroids). weighted=True: mlhip_kmeans_step_weighted on the attached
        weights (set_weights) -- weighted inertia, counts and means; n_changed, labels and distances stay per row."""
        centroids = self._centroids(centroids)
        K = centroids.shape[0]
        inertia, changed = C.c_double(), C.c_uint64()
        counts, cout = np.empty(K), np.empty((K, self.d))
        step = lib.mlhip_kmeans_step_weighted if weighted else lib.mlhip_kmeans_step
        check(step(self.ctx.handle, self._h, K, dptr(centroids), C.byref(inertia), C.byref(changed), dptr(counts), dptr(cout)))
        return inertia.value, changed.value, counts, cout

    def kmeans_iterate(self, centroids, max_steps, atol=0.0, weighted=False):
        """The step loop of KMeans::fit_once in one call (mlhip_kmeans_iterate): the centroid table stays on the device
        between steps. Returns (steps_done, converged, inertia, counts, centroids, old_centroids). weighted=True: the loop of
        weighted steps (mlhip_kmeans_iterate_weighted)."""
        cur = self._centroids(centroids, copy=True)
        K = cur.shape[0]
        old, counts = np.zeros((K, self.d)), np.zeros(K)
        steps, conv, inertia = C.c_uint32(), C.c_int(), C.c_double()
        iterate = lib.mlhip_kmeans_iterate_weighted if weighted else lib.mlhip_kmeans_iterate
        check(iterate(self.ctx.handle, self._h, K, dptr(cur), dptr(old), max_steps, atol, C.byref(steps), C.byref(conv), C.byref(inertia),
                      dptr(counts)))
        return steps.value, bool(conv.value), inertia.value, counts, cur, old

    def kmeans_assign(self, centroids, weighted=False):
        """Assignment only: (inertia, n_changed). weighted=True: the weighted inertia (mlhip_kmeans_assign_weighted)."""
        centroids = self._centroids(centroids)
        K = centroids.shape[0]
        inertia, changed = C.c_double(), C.c_uint64()
        assign = lib.mlhip_kmeans_assign_weighted if weighted else lib.mlhip_kmeans_assign
        check(assign(self.ctx.handle, self._h, K, dptr(centroids), C.byref(inertia), C.byref(changed)))
        return inertia.value, changed.value

    def kmeans_labels(self):
        out = np.empty(self.n, dtype=np.uint32)
        check(lib.mlhip_kmeans_labels(self.ctx.handle, self._h, u32ptr(out)))
        return out

    def kmeans_distances(self):
        """Per-sample squared distance to the assigned centroid from the last assignment."""
        out = np.empty(self.n)
        check(lib.mlhip_kmeans_distances(self.ctx.handle, self._h, dptr(out)))
        return out

    def min_squared_distances(self, centroids):
        centroids = self._centroids(centroids)
        out = np.empty(self.n)
        check(lib.mlhip_min_squared_distances(self.ctx.handle, self._h, centroids.shape[0], dptr(centroids), dptr(out)))
        return out


def silhouette(data, labels, K=None, rows=None, parts=False):
    """Exact silhouette values (Euclidean) of the rows of the Data block `data` under `labels` (mlhip_silhouette): one float64 per
    row, or per entry of `rows` (row indices, any order, repeats allowed), every one scored against ALL rows of the block.
    parts=True: the tuple (a, b, s) -- mean distance to the row's own cluster, to the nearest other cluster, and the silhouette value.
    labels: one integer in [0, K) per row (K: max + 1 unless given). Weights attached to the block play no part. TypeError /
    ValueError before any device work: see silhouette_arguments. A function of the module, not a method of Data; nothing the handle
    holds is changed."""
    labels, K, rows = silhouette_arguments(data.n, labels, rows, K)
    m = data.n if rows is None else len(rows)
    s = np.empty(m)
    a = np.empty(m) if parts else None
    b = np.empty(m) if parts else None
    check(lib.mlhip_silhouette(data.ctx.handle, data._h, K, u32ptr(labels), None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                               m, dptr(a), dptr(b), dptr(s)))
    return (a, b, s) if parts else s


def silhouette_route(data):
    """The tier mlhip_silhouette runs on the Data block `data` under the switches as they are set now (mlhip_silhouette_route):
    'registers' | 'plain'."""
    return _route_name(lib.mlhip_silhouette_route, ("registers", "plain"), data._h)


def silhouette_arguments(n, labels, rows=None, K=None):
    """The argument checks of the silhouette calls, before any device work: returns (labels as a C-contiguous uint32 array of length
    n, K, rows as a C-contiguous uint64 array or None). labels: a 1-D integer array or a list of n integers >= 0 (K: max + 1 unless
    given, then every label < K), at least two distinct values among them; rows: None or 1-D integers in [0, n). TypeError for
    another type or dtype, ValueError for a wrong length or refused values."""
    def integers(v, what):
        arr = np.asarray(v)
        if arr.dtype == object or not (np.issubdtype(arr.dtype, np.integer) or (arr.size == 0 and isinstance(v, (list, tuple)))):
            raise TypeError(f"{what} must be integers (a 1-D integer array or a list of them)")
        if arr.ndim != 1:
            raise ValueError(f"{what} must be one-dimensional")
        return arr
    labels = integers(labels, "labels")
    if len(labels) != n:
        raise ValueError(f"labels has {len(labels)} entries for {n} rows")
    if n and labels.min() < 0:
        raise ValueError("labels must be >= 0")
    top = int(labels.max()) + 1 if n else 0
    if K is None:
        K = top
    K = int(K)
    if top > K:
        raise ValueError("a label is not below K")
    if K > 0xffffffff:
        raise ValueError("labels must be below 2^32")
    if n == 0 or len(np.unique(labels)) < 2:
        raise ValueError("the silhouette needs at least two non-empty clusters")
    if rows is not None:
        rows = integers(rows, "rows")
        if len(rows) and (rows.min() < 0 or rows.max() >= n):
            raise ValueError("a row index is outside [0, N)")
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
    return np.ascontiguousarray(labels, dtype=np.uint32), K, rows


def silhouette_finish(counts, own_label, sums):
    """The closing arithmetic of the silhouette for one row on the host (mlhip_silhouette_finish, device/silhouette_finish.hpp
    compiled for the host; no GPU): counts -- the K cluster sizes, own_label -- the row's label, sums -- its K sums of distances.
    Returns (a, b, s)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    if counts.ndim != 1:
        raise ValueError(f"counts has shape {counts.shape}, expected (K,)")
    _require_shape("sums", sums, *counts.shape)
    a, b, s = C.c_double(), C.c_double(), C.c_double()
    check(lib.mlhip_silhouette_finish(len(counts), counts.ctypes.data_as(C.POINTER(C.c_uint64)), int(own_label), dptr(sums), C.byref(a),
                                      C.byref(b), C.byref(s)))
    return a.value, b.value, s.value


def calculate_XXt_beta(X, y, lam):
    """ml::LinearRegression::calculate_XXt_beta on an N x q float64 C-contiguous X: returns (XXt + diag(lam), beta)."""
    if not _is_block(X):
        raise TypeError("X must be a C-contiguous float64 N x q numpy array")
    y = np.ascontiguousarray(y, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    n, q = X.shape
    XXt, beta = np.empty((q, q)), np.empty(q)
    check(lib.mlpp_calculate_XXt_beta(dptr(X), n, q, dptr(y), y.size, dptr(lam), lam.size, dptr(XXt), dptr(beta)))
    return XXt, beta


def finalize_statistics_ridge(statistics, shift, n_global, ridge):
    """The full M-step's closing arithmetic on the host with the covariance ridge given (mlhip_em_finalize_statistics_ridge, no GPU):
    statistics K x (d+1)(d+2)/2 packed records. Returns (mixing, means K x d, covariances K x d x d)."""
    st = np.ascontiguousarray(statistics, dtype=np.float64)
    shift = np.ascontiguousarray(shift, dtype=np.float64)
    K, d = st.shape[0], shift.shape[0]
    _require_shape("statistics", st, K, (d + 1) * (d + 2) // 2)
    pi, mu, S = np.empty(K), np.empty((K, d)), np.empty((K, d, d))
    check(lib.mlhip_em_finalize_statistics_ridge(d, K, dptr(st), dptr(shift), n_global, ridge, dptr(pi), dptr(mu), dptr(S)))
    return pi, mu, S


def finalize_statistics_tied(statistics, total_scatter, shift, total_weight, ridge=None):
    """The tied M-step's closing arithmetic on the host (mlhip_em_finalize_statistics_tied, no GPU): statistics K x (d + 1) rows
    [S1_k | S0_k], total_scatter the packed (d+1)(d+2)/2 lower triangle of sum_i w_i [x~_i; 1][x~_i; 1]^T. Returns
    (mixing, means K x d, covariance d x d). `ridge`: the covariance ridge (mlhip_em_finalize_statistics_tied_ridge); None: the default."""
    st = np.ascontiguousarray(statistics, dtype=np.float64)
    K, d = st.shape[0], st.shape[1] - 1
    T = np.ascontiguousarray(total_scatter, dtype=np.float64)
    shift = np.ascontiguousarray(shift, dtype=np.float64)
    _require_shape("total_scatter", T, (d + 1) * (d + 2) // 2)
    _require_shape("shift", shift, d)
    pi, mu, S = np.empty(K), np.empty((K, d)), np.empty((d, d))
    if ridge is None:
        check(lib.mlhip_em_finalize_statistics_tied(d, K, dptr(st), dptr(T), dptr(shift), total_weight, dptr(pi), dptr(mu), dptr(S)))
    else:
        check(lib.mlhip_em_finalize_statistics_tied_ridge(d, K, dptr(st), dptr(T), dptr(shift), total_weight, ridge, dptr(pi), dptr(mu), dptr(S)))
    return pi, mu, S


def cholesky_lower(cov):
    """The lower Cholesky factor the sampler uses (mlhip_cholesky_lower, no GPU): L with L @ L.T == cov up to rounding, upper
    triangle zero. ValueError when cov is not positive definite."""
    cov = np.ascontiguousarray(cov, dtype=np.float64)
    d = len(cov)
    _require_shape("cov", cov, d, d)
    L = np.empty((d, d), order="F")
    check(lib.mlhip_cholesky_lower(d, dptr(cov), dptr(L)))
    return np.ascontiguousarray(L)


def em_condition(means, covs, observed, diagonal=False, tied=False):
    """A mixture over (x_O, x_M) conditioned on the coordinates `observed` (mlhip_em_condition, no GPU): (means_observed K x dO,
    covs_observed K x dO x dO, maps K x dM x dO, means_missing K x dM), the missing coordinates in ascending order. means: K x d;
    covs: K x d x d (K x d variances with diagonal=True, the one d x d matrix with tied=True). ValueError for bad coordinates or an
    observed block that is not positive definite."""
    K, d, mode, _, means, covs = mixture_arguments(None, means, covs, diagonal, tied)
    observed = np.ascontiguousarray(observed, dtype=np.uint32).ravel()
    dO = len(observed)
    dM = max(d - dO, 0)
    mu_o, S_oo, A, mu_m = np.empty((K, dO)), np.empty((K, dO, dO)), np.empty((K, dM, dO)), np.empty((K, dM))
    check(lib.mlhip_em_condition(d, K, mode, dptr(means), dptr(covs), u32ptr(observed), dO, dptr(mu_o), dptr(S_oo), dptr(A), dptr(mu_m)))
    return mu_o, S_oo, A, mu_m


def _impute_block(x, d=None):
    if not _is_block(x):
        raise TypeError("x must be a C-contiguous float64 N x d numpy array")
    if d is not None and x.shape[1] != d:
        raise ValueError(f"x must have one column per coordinate of the model ({d})")
    return x


def em_impute(ctx, mixing, means, covs, x, diagonal=False, tied=False, log_density=False, responsibilities=False):
    """x (N x d C-contiguous float64, NaN = missing, every row its own pattern) with every NaN replaced by its conditional expectation
    under the mixture given the coordinates the row has (mlhip_em_impute): a new N x d array, observed entries bit for bit -- with
    log_density=True and / or responsibilities=True a tuple of it, the N log-densities of the rows' observed coordinates under the
    marginal mixture and the N x K marginal responsibilities (C-contiguous), in that order. ctx: a Context or a device group (every
    shard imputes its own rows). means: K x d; covs as for Data.em_score. TypeError / ValueError before any device work; ValueError
    where the observed block of a covariance is not positive definite for some row's pattern (nothing is returned)."""
    K, d, mode, mixing, means, covs = mixture_arguments(mixing, means, covs, diagonal, tied)
    x = _impute_block(x, d)
    n = x.shape[0]
    out = np.empty((n, d))
    dens = np.empty(n) if log_density else None
    resp = np.empty((n, K)) if responsibilities else None
    check(lib.mlhip_em_impute(ctx.handle, d, K, mode, dptr(mixing), dptr(means), dptr(covs), dptr(x), n, dptr(out), dptr(dens), dptr(resp)))
    return _with_optional(out, dens, resp)


def em_impute_plan(x):
    """The pattern grouping mlhip_em_impute makes of x (mlhip_em_impute_plan, no GPU): (order, bounds, n_observed) -- the rows in a
    stable order in which the rows of one pattern of NaNs are contiguous and ascending (uint32, N), the P + 1 group bounds into it and
    the number of observed coordinates of each of the P patterns."""
    x = _impute_block(x)
    n, d = x.shape
    order, bounds, n_obs = np.empty(n, dtype=np.uint32), np.empty(n + 1, dtype=np.uint32), np.empty(n, dtype=np.uint32)
    p = C.c_uint32()
    check(lib.mlhip_em_impute_plan(dptr(x), n, d, C.byref(p), u32ptr(order), u32ptr(bounds), u32ptr(n_obs)))
    return order, bounds[:p.value + 1].copy(), n_obs[:p.value].copy()


def em_impute_route(d, K, x=None):
    """The route mlhip_em_impute takes for a d-dimensional model of K components under the switches as they are set now
    (mlhip_em_impute_route, no GPU, nothing is launched): 'composed' | 'kernel' -- with a block x a pair of it and the kernel launches
    the call makes for that block."""
    if x is None:
        return _route_name(lib.mlhip_em_impute_route, ("composed", "kernel"), d, K, None, 0, after=(None,))
    x = _impute_block(x, d)
    launches = C.c_uint64()
    route = _route_name(lib.mlhip_em_impute_route, ("composed", "kernel"), d, K, dptr(x), len(x), after=(C.byref(launches),))
    return route, launches.value


def em_impute_condition(ctx, mixing, means, covs, observed, diagonal=False, tied=False):
    """The records the kernel route of mlhip_em_impute builds ON THE DEVICE for the pattern that observes the ascending coordinates
    `observed` (mlhip_em_impute_condition; d <= 32): (means_observed K x dO, whitening K x dO x dO -- W_k = L^-1, L L^T = Sigma_k,OO --,
    coefficients K -- log pi_k - sum_j log L_jj --, maps K x dM x dO, means_missing K x dM). ValueError for bad coordinates or an
    observed block that is not positive definite."""
    K, d, mode, mixing, means, covs = mixture_arguments(mixing, means, covs, diagonal, tied)
    observed = np.ascontiguousarray(observed, dtype=np.uint32).ravel()
    dO = len(observed)
    dM = max(d - dO, 0)
    mu_o, W, coef, A, mu_m = np.empty((K, dO)), np.empty((K, dO, dO)), np.empty(K), np.empty((K, dM, dO)), np.empty((K, dM))
    check(lib.mlhip_em_impute_condition(ctx.handle, d, K, mode, dptr(mixing), dptr(means), dptr(covs), u32ptr(observed), dO, dptr(mu_o),
                                        dptr(W), dptr(coef), dptr(A), dptr(mu_m)))
    return mu_o, W, coef, A, mu_m


def em_condition_covariances(covs, observed, diagonal=False, tied=False, K=None):
    """The covariances of the components of a mixture conditioned on the coordinates `observed` and their lower Cholesky factors
    (mlhip_em_condition_covariances, no GPU): (covariances_missing K x dM x dM, factors K x dM x dM, zero above the diagonal), the
    missing coordinates in ascending order. covs as for em_condition (tied=True: the one d x d matrix, and K components). ValueError for
    bad coordinates or a block that is not positive definite."""
    covs = np.ascontiguousarray(covs, dtype=np.float64)
    if tied and K is None:
        raise ValueError("tied=True needs K, the number of components")
    if covs.ndim < 2:
        raise ValueError(f"covs has shape {covs.shape}: not the covariances of a mixture")
    K, d = (K, covs.shape[0]) if tied else covs.shape[:2]
    _require_shape("covs", covs, *_covariance_shape(K, d, diagonal, tied))
    observed = np.ascontiguousarray(observed, dtype=np.uint32).ravel()
    dM = max(d - len(observed), 0)
    C_m, G = np.empty((K, dM, dM)), np.empty((K, dM, dM))
    check(lib.mlhip_em_condition_covariances(d, K, 2 if tied else int(bool(diagonal)), dptr(covs), u32ptr(observed), len(observed), dptr(C_m),
                                             dptr(G)))
    return C_m, G


def em_conditional_variances(data, mixing, means_observed, covs_observed, maps, means_missing, covs_missing, full=False, means=False,
                             log_density=False):
    """Var[x_M | x_O] for every row of `data`, a Data block of OBSERVED coordinates, under the conditioned mixture em_condition and
    em_condition_covariances return (mlhip_em_conditional_variances): n x dM C-contiguous float64, or n x dM x dM with full=True. With
    means=True and / or log_density=True a tuple of it, E[x_M | x_O] (n x dM) and the n log-densities of the rows under the marginal
    mixture, in that order -- the bits of Data.em_conditional_means. covs_missing: K x dM x dM, the other parameters as for
    Data.em_conditional_means. A function of the module, not a method of Data; nothing the handle holds is changed."""
    K, dM, arrays = conditioned_arguments(data.d, mixing, means_observed, covs_observed, maps, means_missing, covs_missing=covs_missing)
    out = np.empty((data.n, dM, dM) if full else (data.n, dM))
    y = np.empty((data.n, dM)) if means else None
    dens = np.empty(data.n) if log_density else None
    check(lib.mlhip_em_conditional_variances(data.ctx.handle, data._h, K, dM, *map(dptr, arrays), bool(full), dptr(out),
                                             dM * dM if full else dM, dptr(y), dM, dptr(dens)))
    return _with_optional(out, y, dens)


def em_condition_variance_route(data, K, dM, full=False):
    """The kernel mlhip_em_conditional_variances runs for dM missing coordinates on the Data block `data` in the form asked for, under
    the switches as they are set now (mlhip_em_condition_variance_route): 'registers' | 'plain'."""
    return _route_name(lib.mlhip_em_condition_variance_route, ("registers", "plain"), data._h, K, dM, bool(full))


def normal_cdf(a):
    """The standard normal CDF the conditional CDF / quantile kernels use (mlhip_normal_cdf, device/normal_cdf.hpp compiled for the
    host; no GPU), elementwise: float64, the shape of `a`."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    check(lib.mlhip_normal_cdf(dptr(a), a.size, dptr(out)))
    return out


def normal_quantile(p):
    """The inverse of normal_cdf (mlhip_normal_quantile, no GPU), elementwise; ValueError for a probability that is a NaN or not
    strictly inside (0, 1)."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    out = np.empty_like(p)
    check(lib.mlhip_normal_quantile(dptr(p), p.size, dptr(out)))
    return out


QUANTILE_MAX_TRIPS = 84      # MLHIP_QUANTILE_MAX_TRIPS: the trip cap of the quantile search


def em_condition_scales(covs_missing):
    """(scales, inverse_scales), K x dM each: s_kj = sqrt(C_k[j][j]) and w_kj = 1.0 / s_kj from the K x dM x dM conditioned covariances
    of em_condition_covariances (mlhip_em_condition_scales, no GPU). ValueError where a C_k[j][j] is <= 0 or not finite."""
    covs_missing = np.ascontiguousarray(covs_missing, dtype=np.float64)
    if covs_missing.ndim != 3 or covs_missing.shape[1] != covs_missing.shape[2]:
        raise ValueError(f"covs_missing has shape {covs_missing.shape}, expected (K, dM, dM)")
    K, dM = covs_missing.shape[:2]
    s, w = np.empty((K, dM)), np.empty((K, dM))
    check(lib.mlhip_em_condition_scales(K, dM, dptr(covs_missing), dptr(s), dptr(w)))
    return s, w


def em_conditional_cdfs(data, mixing, means_observed, covs_observed, maps, means_missing, scales, inverse_scales, values, means=False,
                        log_density=False):
    """P(x_j <= values[i, j] | x_O) per missing coordinate for every row of `data`, a Data block of OBSERVED coordinates, under the
    conditioned mixture em_condition returns and the scales of em_condition_scales (mlhip_em_conditional_cdfs): n x dM C-contiguous
    float64. With means=True and / or log_density=True a tuple of it, E[x_M | x_O] (n x dM) and the n log-densities of the rows under
    the marginal mixture, in that order -- the bits of Data.em_conditional_means. A function of the module, not a method of Data;
    nothing the handle holds is changed."""
    K, dM, arrays = conditioned_arguments(data.d, mixing, means_observed, covs_observed, maps, means_missing, scales=scales,
                                          inverse_scales=inverse_scales)
    values = np.ascontiguousarray(values, dtype=np.float64)
    _require_shape("values", values, data.n, dM)
    out = np.empty((data.n, dM))
    y = np.empty((data.n, dM)) if means else None
    dens = np.empty(data.n) if log_density else None
    check(lib.mlhip_em_conditional_cdfs(data.ctx.handle, data._h, K, dM, *map(dptr, arrays), dptr(values), dM, dptr(out), dM, dptr(y), dM,
                                        dptr(dens)))
    return _with_optional(out, y, dens)


def em_conditional_quantiles(data, mixing, means_observed, covs_observed, maps, means_missing, scales, inverse_scales, probabilities,
                             iterations=False, means=False, log_density=False):
    """The quantiles of x_j | x_O per missing coordinate at every probability (each strictly inside (0, 1)) for every row of `data`
    (mlhip_em_conditional_quantiles): P x n x dM C-contiguous float64, probability-major. With iterations=True, means=True and / or
    log_density=True a tuple of it, the trips every output took (P x n x dM uint32), E[x_M | x_O] and the log-densities, in that
    order. Arguments as for em_conditional_cdfs. ValueError for a bad probability, before any device work."""
    K, dM, arrays = conditioned_arguments(data.d, mixing, means_observed, covs_observed, maps, means_missing, scales=scales,
                                          inverse_scales=inverse_scales)
    probabilities = np.ascontiguousarray(probabilities, dtype=np.float64)
    if probabilities.ndim != 1:
        raise ValueError(f"probabilities has shape {probabilities.shape}, expected (P,)")
    P = len(probabilities)
    out = np.empty((P, data.n, dM))
    trips = np.zeros((P, data.n, dM), dtype=np.uint32) if iterations else None
    y = np.empty((data.n, dM)) if means else None
    dens = np.empty(data.n) if log_density else None
    check(lib.mlhip_em_conditional_quantiles(data.ctx.handle, data._h, K, dM, *map(dptr, arrays), dptr(probabilities), P, dptr(out), dM,
                                             dptr(y), dM, dptr(dens), u32ptr(trips)))
    return _with_optional(out, trips, y, dens)


def em_condition_quantile_route(data, K, dM, quantile=True):
    """The kernel mlhip_em_conditional_quantiles (quantile=True) or mlhip_em_conditional_cdfs (quantile=False) runs for dM missing
    coordinates on the Data block `data`, under the switches as they are set now (mlhip_em_condition_quantile_route): 'registers' |
    'plain'."""
    return _route_name(lib.mlhip_em_condition_quantile_route, ("registers", "plain"), data._h, K, dM, bool(quantile))


def em_sample_route(d, K):
    """The kernel the sampling calls run for K components in d dimensions under the switches as they are set now
    (mlhip_em_sample_route): 'lds_table' | 'global_table' | 'plain'."""
    return _route_name(lib.mlhip_em_sample_route, ("lds_table", "global_table", "plain"), d, K)


def process_covariance(cov):
    cov = np.ascontiguousarray(cov, dtype=np.float64)
    d = cov.shape[0]
    inv, sd = np.empty((d, d)), C.c_double()
    check(lib.mlhip_process_covariance(d, dptr(cov), dptr(inv), C.byref(sd)))
    return inv, sd.value
