"""The Python binding's prototypes and argument normalisers. CPU only.

ml_amd/_lib.py reads include/mlhip.h and include/mlpp_c.h when it loads the library and sets restype / argtypes on every function
they declare; mixture_arguments and conditioned_arguments check every argument bundle before a call is made."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_abi_exports import ROOT, declared_functions

HEADERS = ("mlhip.h", "mlpp_c.h")
DP, U32P, U64P, IP, VP = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_void_p


def parameter_counts(header):
    """name -> number of parameters, counted from the declaration's text by its commas; (void) counts as 0."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    counts = {}
    for name, parameters in re.findall(r"\b(ml(?:hip|pp)_[a-zA-Z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        if not name.endswith("_fn"):
            counts[name] = 0 if parameters.strip() == "void" else len(parameters.split(","))
    return counts


@pytest.mark.parametrize("header", HEADERS)
def test_every_declared_function_has_a_prototype(header):
    from ml_amd import _lib
    names, counts = declared_functions(header), parameter_counts(header)
    assert len(names) > 20 and set(names) == set(counts)
    for name in names:
        argtypes = getattr(_lib.lib, name).argtypes
        assert argtypes is not None, name
        assert len(argtypes) == counts[name], name


def test_prototypes_written_out():
    from ml_amd import _lib
    u32, u64, i64, dbl, i = C.c_uint32, C.c_uint64, C.c_int64, C.c_double, C.c_int
    expected = {
        "mlhip_data_upload": [VP, DP, u32, u64, i64, VP],
        "mlhip_em_iterate": [VP, VP, u32, i, DP, DP, DP, u32, dbl, dbl, U32P, IP, DP, DP],
        "mlhip_em_screen_counts": [VP, VP, U64P],
        "mlhip_ctx_set_allreduce": [VP, _lib.ALLREDUCE_FN, VP, i, i, i],
        "mlhip_ctx_reduce_kind": [VP, C.POINTER(C.c_char_p)],
        "mlhip_ctx_init_rccl_file": [VP, C.c_char_p, i, i],
        "mlhip_ctx_allreduce": [VP, DP, C.c_size_t],
        "mlhip_em_route": [VP, u32, i, C.POINTER(_lib.EmRouteInfo)],
        "mlhip_kmeans_route": [VP, u32, C.POINTER(_lib.KmeansRouteInfo)],
        "mlhip_silhouette": [VP, VP, u32, U32P, U64P, u64, DP, DP, DP],
        "mlhip_last_error": [],
        "mlpp_em_fit_weighted": [VP, DP, DP, u64, u32, IP],
        "mlpp_device_context": [VP],
        "mlhip_em_finalize_statistics_ridge": [u32, u32, DP, DP, dbl, dbl, DP, DP, DP],
    }
    for name, argtypes in expected.items():
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is (C.c_char_p if name == "mlhip_last_error" else C.c_int), name
    assert _lib.lib.mlhip_version.restype is C.c_char_p


def test_scalars_by_value_convert_as_declared():
    from ml_amd import _lib
    d, K, n = 2, 2, 50
    rng = np.random.default_rng(3)
    Z = np.hstack([rng.standard_normal((n, d)), np.ones((n, 1))])
    R = rng.dirichlet(np.ones(K), size=n)
    st = np.array([[((Z * R[:, k][:, None]).T @ Z)[a, b] for a in range(d + 1) for b in range(a + 1)] for k in range(K)])
    shift = np.array([0.25, -1.5])
    want = _lib.finalize_statistics_ridge(st, shift, float(n), 1e-6)
    got = np.empty(K), np.empty((K, d)), np.empty((K, d, d))
    call = lambda K_: _lib.lib.mlhip_em_finalize_statistics_ridge(d, K_, _lib.dptr(st), _lib.dptr(shift), float(n), 1e-6, *map(_lib.dptr, got))
    assert call(K) == _lib.OK
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    with pytest.raises(C.ArgumentError):
        call(1.5)


def mixture(K=3, d=2, R=None):
    lead = () if R is None else (R,)
    full = np.broadcast_to(np.eye(d), lead + (K, d, d)).copy()
    return {"mixing": np.full(lead + (K,), 1.0 / K), "means": np.arange(np.prod(lead + (K, d)), dtype=np.float64).reshape(lead + (K, d)),
            "full": full, "diag": np.ones(lead + (K, d)), "tied": np.broadcast_to(np.eye(d), lead + (d, d)).copy()}


@pytest.mark.parametrize("R", [None, 2])
def test_mixture_arguments(R):
    from ml_amd import _lib
    m, lead, restarts = mixture(R=R), (() if R is None else (R,)), R is not None
    for code, (mode, flags) in enumerate([("full", {}), ("diag", {"diagonal": True}), ("tied", {"tied": True})]):
        K, d, covariance_type, *arrays = _lib.mixture_arguments(m["mixing"], m["means"], m[mode], restarts=restarts, **flags)
        assert (K, d, covariance_type) == (3, 2, code)
        assert all(a.flags.c_contiguous and a.dtype == np.float64 for a in arrays)
        assert arrays[2].shape == m[mode].shape and np.array_equal(arrays[1], m["means"])
    # converted where they must be
    _, _, _, pi, mu, S = _lib.mixture_arguments(m["mixing"].astype(np.float32), np.asfortranarray(m["means"]), np.asfortranarray(m["full"]),
                                                d=2, restarts=restarts)
    assert all(a.flags.c_contiguous and a.dtype == np.float64 for a in (pi, mu, S))
    assert np.array_equal(mu, m["means"]) and np.array_equal(S, m["full"])
    # copy=True: fresh arrays
    copies = _lib.mixture_arguments(m["mixing"], m["means"], m["full"], copy=True, restarts=restarts)[3:]
    assert not any(np.shares_memory(a, b) for a, b in zip(copies, (m["mixing"], m["means"], m["full"])))
    refused = [
        dict(mixing=np.full(lead + (2,), 0.5), means=m["means"], covs=m["full"]),
        dict(mixing=m["mixing"], means=np.zeros(lead + (3, 3)), covs=m["full"], d=2),
        dict(mixing=m["mixing"], means=m["means"], covs=m["diag"]),
        dict(mixing=m["mixing"], means=m["means"], covs=m["full"], diagonal=True),
        dict(mixing=m["mixing"], means=m["means"], covs=m["full"], tied=True),
        dict(mixing=m["mixing"], means=m["means"], covs=m["full"], diagonal=True, tied=True),
    ]
    for arguments in refused:
        with pytest.raises(ValueError):
            _lib.mixture_arguments(restarts=restarts, **arguments)
    with pytest.raises(ValueError):                               # the restart axis itself: missing, or there unasked
        _lib.mixture_arguments(m["mixing"], m["means"], m["full"], restarts=not restarts)


def test_conditioned_arguments():
    from ml_amd import _lib
    K, dO, dM = 2, 2, 1
    right = dict(mixing=np.full(K, 0.5), means_observed=np.zeros((K, dO)), covs_observed=np.stack([np.eye(dO)] * K), maps=np.ones((K, dM, dO)),
                 means_missing=np.zeros((K, dM)))
    extra = dict(factors=np.ones((K, dM, dM)), covs_missing=np.ones((K, dM, dM)), scales=np.ones((K, dM)), inverse_scales=np.ones((K, dM)))
    got_K, got_dM, arrays = _lib.conditioned_arguments(dO, **right)
    assert (got_K, got_dM, len(arrays)) == (K, dM, 5)
    got_K, got_dM, arrays = _lib.conditioned_arguments(dO, **right, **extra)
    assert (got_K, got_dM, len(arrays)) == (K, dM, 9)
    assert all(a.flags.c_contiguous and a.dtype == np.float64 for a in arrays)
    assert arrays[3].shape == (K, dM, dO) and arrays[5].shape == (K, dM, dM) and arrays[8].shape == (K, dM)
    with pytest.raises(ValueError, match="maps"):
        _lib.conditioned_arguments(dO, **{**right, "maps": np.ones((2, 2, 1))})
    with pytest.raises(ValueError, match="factors"):
        _lib.conditioned_arguments(dO, **right, factors=np.ones((2, 2, 2)))
    with pytest.raises(ValueError, match="scales"):
        _lib.conditioned_arguments(dO, **right, scales=np.ones(2), inverse_scales=np.ones((K, dM)))


def test_an_unmappable_declaration_is_refused():
    from ml_amd import _lib
    good = "/* a comment */\nint mlhip_fine(const double* x, uint64_t n);\nconst char* mlhip_name(void);\n"
    assert _lib._prototypes(good) == {"mlhip_fine": (C.c_int, [DP, C.c_uint64]), "mlhip_name": (C.c_char_p, [])}
    with pytest.raises(ImportError) as e:
        _lib._prototypes(good + "int mlhip_odd(mlhip_ctx* ctx, float* values);\n")
    assert "mlhip_odd" in str(e.value) and "float*" in str(e.value)
    with pytest.raises(ImportError, match="mlhip_returns"):
        _lib._prototypes("double mlhip_returns(void);\n")
