"""gc_array_covariance / gc_array_combine at the boundary, without a GPU: declared in include/gnsscorr.h, exported by the library,
bound by _lib.py with the declared argument types; the three structs field by field with the sizes (24, 32, 16) and offsets the C
compiler gives them; the two constants the same on both sides; the API version unchanged; Engine.array_covariance / array_combine
refuse records, weights and numbers that do not fit before any library call; the MEX gateway lists and handles the two commands;
and the host arithmetic between the two calls (receiver.array_covariance_matrix, power_inversion_weights, mvdr_weights) against direct
sums and closed forms."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnsscorr.h")
STRUCTS = {"gc_array_cov_params": ["first_sample", "nsamples", "nrecords", "nlags"],
           "gc_array_combine_params": ["first_sample", "noutputs", "dst_first", "nrecords", "ntaps"],
           "gc_array_combine_result": ["clipped", "sum_sq"]}
SIZES = {"gc_array_cov_params": 24, "gc_array_combine_params": 32, "gc_array_combine_result": 16}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, f"include/gnsscorr.h does not declare {name}"
    return [re.sub(r"\s*\w+$", "", " ".join(p.split())).replace(" *", "*") for p in m.group(1).split(",")]


def test_header_declares_the_calls_and_the_binding_has_their_argument_types():
    from cu_sdr_collection_amd import _lib as L
    ctypes_of = {"gc_context* const*": C.POINTER(C.c_void_p), "gc_context*": C.c_void_p, "const gc_array_cov_params*": C.POINTER(L.gc_array_cov_params),
                 "int64_t*": C.POINTER(C.c_int64), "const gc_array_combine_params*": C.POINTER(L.gc_array_combine_params),
                 "const double*": C.POINTER(C.c_double), "gc_array_combine_result*": C.POINTER(L.gc_array_combine_result)}
    cov = ["gc_context* const*", "const gc_array_cov_params*", "int64_t*"]
    comb = ["gc_context* const*", "gc_context*", "const gc_array_combine_params*", "const double*", "gc_array_combine_result*"]
    assert _params("gc_array_covariance") == cov and _params("gc_array_combine") == comb
    lib = L.load()
    for name, params in (("gc_array_covariance", cov), ("gc_array_combine", comb)):
        res, args = L.SYMBOLS[name]
        assert res is C.c_int and args == [ctypes_of[p] for p in params], name
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args
    assert lib.gc_api_version() == 4                      # an addition, not a break
    assert re.search(r"\blong long\s+gc_debug_array_tile_outputs\s*\(\s*int\s+nrecords\s*,\s*int\s+ntaps\s*\)\s*;", _header())
    assert L.SYMBOLS["gc_debug_array_tile_outputs"] == (C.c_longlong, [C.c_int, C.c_int])
    assert lib.gc_debug_array_tile_outputs(8, 32) >= 1024 and lib.gc_debug_array_tile_outputs(1, 1) >= 1024
    assert lib.gc_debug_array_tile_outputs(0, 1) == lib.gc_debug_array_tile_outputs(9, 1) == lib.gc_debug_array_tile_outputs(1, 0) == 0
    assert lib.gc_debug_array_tile_outputs(1, 33) == 0
    # a null argument is refused before any device is looked for
    assert lib.gc_array_covariance(None, None, None) == L.GC_E_INVALID
    assert lib.gc_array_combine(None, None, None, None, None) == L.GC_E_INVALID


def test_structs_and_the_constants_are_the_same_on_both_sides_and_as_the_c_compiler_sees_them():
    from cu_sdr_collection_amd import _lib as L
    h = _header()
    m = re.search(r"#define\s+GC_ARRAY_MAX_RECORDS\s+(\d+)", h)
    assert m and int(m.group(1)) == L.GC_ARRAY_MAX_RECORDS == 8
    m = re.search(r"#define\s+GC_ARRAY_MAX_TAPS\s+(\d+)", h)
    assert m and int(m.group(1)) == L.GC_ARRAY_MAX_TAPS == 32
    assert re.search(r"#define\s+GC_API_VERSION\s+4\b", h)
    for name, fields in STRUCTS.items():
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), h, flags=re.S)
        assert body, name
        declared = [f for decl in body.group(1).split(";") if decl.strip() for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
        assert declared == fields == [f for f, _ in getattr(L, name)._fields_], name
    lines = ['printf("%d %d %d\\n", GC_ARRAY_MAX_RECORDS, GC_ARRAY_MAX_TAPS, GC_API_VERSION);']
    for name, fields in STRUCTS.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % name)
        lines += ['printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, f, name, f) for f in fields]
    prog = "#include <stddef.h>\n#include <stdio.h>\n#include \"gnsscorr.h\"\nint main(void) {\n  %s\n  return 0;\n}\n" % "\n  ".join(lines)
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [[int(x) for x in line.split()] for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert got.pop(0) == [8, 32, 4]
    for name, fields in STRUCTS.items():
        cls = getattr(L, name)
        assert got.pop(0) == [C.sizeof(cls)] == [SIZES[name]], name
        for f in fields:
            d = getattr(cls, f)
            assert got.pop(0) == [d.offset, d.size], (name, f)
    assert not got


class _NoLibrary:
    """Stands where a library or a context would: any use is a library call that came too early."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was used ({name}) before the arguments were checked")


def _engine():
    import cu_sdr_collection_amd as P
    eng = object.__new__(P.Engine)                        # no context, no library: a call that got past the checks would fail
    eng._lib = _NoLibrary()
    eng._ctx = None
    return eng


def test_engine_array_calls_refuse_what_does_not_fit_before_any_library_call():
    import cu_sdr_collection_amd as P
    E = P.Engine
    recs = [_engine(), _engine()]
    dst = _NoLibrary()
    for bad in (None, 5, [], [_engine()] * 9, [_engine(), "x"], [_engine(), None]):
        with pytest.raises(ValueError, match="records"):
            E.array_covariance(bad, 0, 100)
        with pytest.raises(ValueError, match="records"):
            E.array_combine(bad, dst, np.ones(2), noutputs=10)
    for name, bad in (("first_sample", 0.5), ("first_sample", "3"), ("first_sample", 1 << 63), ("nsamples", 2.5), ("nsamples", None), ("nsamples", True),
                      ("nlags", 1.5), ("nlags", 1 << 31)):
        with pytest.raises(ValueError, match=name):
            E.array_covariance(recs, **dict(dict(first_sample=0, nsamples=100, nlags=1), **{name: bad}))
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="nlags"):
            E.array_covariance(recs, 0, 100, bad)
    for bad in (np.ones(3), np.ones((3, 2)), np.ones((2, 33)), np.ones((2, 0)), np.ones((2, 3, 3)), np.ones((2, 3, 2), dtype=complex), np.array(["a", "b"]), 1.0,
                np.ones((2, 3, 2, 1))):
        with pytest.raises(ValueError, match="weights"):
            E.array_combine(recs, dst, bad, noutputs=10)
    for name, bad in (("first_sample", 0.5), ("noutputs", 1 << 63), ("noutputs", True), ("dst_first", 1.25), ("dst_first", "0")):
        with pytest.raises(ValueError, match=name):
            E.array_combine(recs, dst, np.ones(2), **dict(dict(first_sample=0, noutputs=10, dst_first=0), **{name: bad}))
    w = E._array_weights([1, 2j], 2)
    assert w.dtype == np.float64 and w.flags.c_contiguous and w.tolist() == [[[1.0, 0.0]], [[0.0, 2.0]]]
    assert E._array_weights(np.array([[1, 2j, 3], [0.5 - 0.25j, 0, 0]]), 2).tolist() == [[[1, 0], [0, 2], [3, 0]], [[0.5, -0.25], [0, 0], [0, 0]]]
    assert E._array_weights(np.ones((8, 32, 2)), 8).shape == (8, 32, 2)
    assert E._whole("array", "nsamples", 7.0, 64) == 7 and E._whole("array", "first_sample", -1, 64) == -1   # the library's to refuse


def test_mex_gateway_lists_and_handles_the_commands():
    text = open(os.path.join(ROOT, "matlab", "gnsscorr_mex.c")).read()
    head = text[:text.index("#include")]
    assert "gnsscorr_mex('array_covariance'" in head and "gnsscorr_mex('array_combine'" in head    # the usage lines in the file's head
    assert 'strcmp(cmd, "array_covariance")' in text and "gc_array_covariance(" in text
    assert 'strcmp(cmd, "array_combine")' in text and "gc_array_combine(" in text
    wrapper = open(os.path.join(ROOT, "matlab", "gnsscorr_null_steer.m")).read()
    assert "gnsscorr_mex('array_covariance'" in wrapper and "gnsscorr_mex('array_combine'" in wrapper


def _direct(z, T, lo, hi):
    """sum over n in [lo, hi) of zz[n] zz[n]^H for the stacked snapshot zz[n] = (z[a][n - s]) at index a T + s"""
    K = z.shape[0]
    R = np.zeros((K * T, K * T), dtype=complex)
    for n in range(lo, hi):
        zz = np.array([z[a][n - s] if n - s >= 0 else 0 for a in range(K) for s in range(T)])
        R += np.outer(zz, np.conj(zz))
    return R


def test_covariance_matrix_against_a_direct_sum():
    """The matrix from the lags is the direct sum over the snapshots wherever the ranges agree: exactly for T = 1, and for T > 1 on
    every entry (a, s), (b, t) up to the edge terms of the range moved back by min(s, t) samples - the min(s, t) products in front
    of the range that the lag sum does not have, and the min(s, t) at its end that it has and the direct sum does not.  A record that
    is zero over those T - 1 samples at either end has no edge terms: exact there too."""
    import array_model as M
    from cu_sdr_collection_amd import receiver as R
    import cu_sdr_collection_amd as P
    assert P.array_covariance_matrix is R.array_covariance_matrix and "null_steer" in P.__all__ and "power_inversion_weights" in P.__all__
    rng = np.random.default_rng(31)
    K, T, n, first = 3, 4, 200, 10
    raws = [rng.integers(-128, 128, 2 * (first + n)).astype(np.int8) for _ in range(K)]
    z = np.array([r[0::2].astype(float) + 1j * r[1::2].astype(float) for r in raws])
    cov = M.covariance(raws, M.IQ, first, n, T)
    got1 = R.array_covariance_matrix(cov, 1)
    assert got1.shape == (K, K) and got1.dtype == np.complex128 and np.array_equal(got1, _direct(z, 1, first, first + n))
    got = R.array_covariance_matrix(cov, T)
    assert got.shape == (K * T, K * T) and np.array_equal(got, np.conj(got.T))                      # Hermitian, to the bit
    want = _direct(z, T, first, first + n)
    for a in range(K):
        for s in range(T):
            for b in range(K):
                for t in range(T):
                    m = min(s, t)                                                                   # the entry's range is [first - m, first + n - m)
                    head = sum(z[a][j - s + m] * np.conj(z[b][j - t + m]) for j in range(first + n - m, first + n))
                    tail = sum(z[a][j - s + m] * np.conj(z[b][j - t + m]) for j in range(first - m, first))
                    # lag sum = direct sum + (the m products at the lag sum's end) - (the m products in front of it), on the moved index
                    assert got[a * T + s, b * T + t] == want[a * T + s, b * T + t] + head - tail, (a, s, b, t)
    # zero over the T - 1 samples at either end: exact on every entry
    for r in raws:
        r[2 * (first - T + 1):2 * first] = 0
        r[2 * (first + n - T + 1):] = 0
    z = np.array([r[0::2].astype(float) + 1j * r[1::2].astype(float) for r in raws])
    assert np.array_equal(R.array_covariance_matrix(M.covariance(raws, M.IQ, first, n, T), T), _direct(z, T, first, first + n))
    with pytest.raises(ValueError, match="cov"):
        R.array_covariance_matrix(cov, T + 1)
    with pytest.raises(ValueError, match="cov"):
        R.array_covariance_matrix(cov[..., 0], 1)


def test_power_inversion_puts_the_null_the_closed_form_says_and_mvdr_keeps_the_look_direction():
    """R = 2 s^2 I + 2 J^2 v v^H with |v_a| = 1 (K elements, one tap).  With c = J^2 / (s^2 + K J^2), the matrix-inversion lemma gives
    R^-1 = (I - c v v^H) / (2 s^2), so R^-1 e = (e - c conj(v_ref) v) / (2 s^2), e^H R^-1 e = (1 - c) / (2 s^2) and
        w = (e - c conj(v_ref) v) / (1 - c),      w^H v = v_ref (1 - c K) / (1 - c) = v_ref s^2 / (s^2 + (K - 1) J^2),
    so |w^H v|^2 = (s^2 / (s^2 + (K - 1) J^2))^2: of the order (s^2 / (K J^2))^2.
    The cases: the solve loses cond(R) = (s^2 + K J^2) / s^2 of float64's 1.1e-16, and w^H v is what is left of terms of size 1 after a
    cancellation by (s^2 + (K - 1) J^2) / s^2; twice the product of the three stays below 1e-12 for the jammed scene of the GPU test
    (s = 8, J = 30, K = 4: 5e-13) and the two others here.  (J / s = 100 at K = 8 would need 1e-10: no case for this bound.)"""
    from cu_sdr_collection_amd import receiver as R
    rng = np.random.default_rng(32)
    for K, s, J, ref in ((4, 8.0, 30.0, 0), (8, 3.0, 6.0, 3), (2, 5.0, 5.0, 1)):
        v = np.exp(1j * rng.uniform(0, 2 * np.pi, K))
        Rm = 2 * s * s * np.eye(K) + 2 * J * J * np.outer(v, np.conj(v))
        w = R.power_inversion_weights(Rm, K, 1, ref=ref)
        assert w.shape == (K,) and abs(w[ref] - 1.0) < 1e-12
        got = abs(np.vdot(w, v)) ** 2                                              # |w^H v|^2
        want = (s * s / (s * s + (K - 1) * J * J)) ** 2
        print(f"power inversion K={K} s={s} J={J}: |w^H v|^2 {got:.17g}, closed form {want:.17g}, relative {abs(got - want) / want:.2e}")
        assert abs(got - want) <= 1e-12 * want, (K, got, want)
        c = J * J / (s * s + K * J * J)
        e = np.zeros(K)
        e[ref] = 1.0
        assert np.max(np.abs(w - (e - c * np.conj(v[ref]) * v) / (1 - c))) < 1e-9
        # loading acts as more noise: 2 s^2 + loading on the diagonal
        wl = R.power_inversion_weights(Rm, K, 1, ref=ref, loading=6 * s * s)
        want_l = (4 * s * s / (4 * s * s + (K - 1) * J * J)) ** 2
        assert abs(abs(np.vdot(wl, v)) ** 2 - want_l) <= 1e-12 * want_l
        # MVDR towards u keeps u and still nulls v
        u = np.exp(1j * rng.uniform(0, 2 * np.pi, K))
        wm = R.mvdr_weights(Rm, u)
        assert abs(np.vdot(wm, u) - 1.0) < 1e-12
    # two taps: the constraint sits at (ref, tap 0)
    A = rng.standard_normal((6, 6)) + 1j * rng.standard_normal((6, 6))
    Rm = A @ np.conj(A.T) + np.eye(6)
    w = R.power_inversion_weights(Rm, 3, 2, ref=1)
    assert abs(w[2] - 1.0) < 1e-12
    for k in range(6):                                                             # least power under the constraint: the gradient along every free direction is 0
        if k != 2:
            assert abs((Rm @ w)[k]) < 1e-9
    with pytest.raises(ValueError):
        R.power_inversion_weights(Rm, 3, 2, ref=3)
    with pytest.raises(ValueError):
        R.power_inversion_weights(Rm[:5], 3, 2)
    with pytest.raises(ValueError):
        R.mvdr_weights(Rm, np.ones(5))
