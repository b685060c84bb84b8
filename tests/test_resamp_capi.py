"""CPU-side checks of the rational resampler's C-ABI boundary (sdsp_resamp_*, include/sdsp.h):
the symbols are exported, create refuses bad arguments in its documented order and a missing
device before any device work, and sdsp_resamp_count (the one piece of index arithmetic every
call runs on) equals a brute-force walk of the decimator's counter.  No compute calls (the
library has no CPU path)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "sdsp.h")

E_COEFFICIENTS_LENGTH_ZERO, E_DECIMATION_LESS_THAN_ONE, E_INTERPOLATION_LESS_THAN_ONE = 1, 2, 3
E_INVALID_ARGUMENT, E_NO_DEVICE = 90, 101


def resamp_symbols():
    text = open(HDR).read()
    return sorted(set(re.findall(r"SDSP_API\s+[\w\s\*]+?\b(sdsp_resamp_\w+)\s*\(", text)))


def test_header_declares_the_resampler_family():
    syms = resamp_symbols()
    names = ("create", "destroy", "clone", "reset", "set_channels", "set_algo", "get_algo", "set_tuning",
             "interpolation", "decimation", "subfilter_len", "get_phase", "set_phase", "output_count",
             "execute_block", "execute_block_device", "info", "synchronize", "count")
    for name in names:
        assert "sdsp_resamp_" + name in syms, name
    assert len(syms) == len(names)  # no per-sample entry point, scale or window get / set
    assert re.search(r"SDSP_TUNE_RESAMP_KERNEL\s*=\s*24\b", open(HDR).read())


def test_library_exports_every_resampler_symbol():
    import solid_dsp_amd as sd
    out = subprocess.run(["nm", "-D", "--defined-only", sd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sdsp_\w+)", out))
    missing = [s for s in resamp_symbols() if s not in exported]
    assert not missing, missing
    lib = sd.lib()  # and the Python loader binds them
    for s in resamp_symbols():
        assert hasattr(lib, s)
    assert sd.Resampler is sd.resamp.Resampler
    assert sd._lib.TUNE_RESAMP_KERNEL == 24


def _create(lib, dtype, coef_dt, len_, M, D, device=0, null_taps=False):
    taps = np.ones(max(len_, 1), dtype=coef_dt)
    h = C.c_void_p(0xdead)  # create must null it on every failure
    p = None if null_taps else taps.ctypes.data_as(C.c_void_p)
    rc = lib.sdsp_resamp_create(C.byref(h), dtype, p, len_, M, D, device)
    return rc, h


def _message(lib):
    m = lib.sdsp_last_error()
    return m.decode() if isinstance(m, bytes) else (m or "")


def test_create_refuses_bad_arguments_in_order():
    """every argument check comes before the device check, so this holds with and without a GPU;
    each call breaks one more rule than the check it expects to fire, so the order shows"""
    import solid_dsp_amd as sd
    lib = sd.lib()
    for dtype in (-1, 6):  # 1. dtype, ahead of null taps, D = 0, len = 0 and M = 0
        rc, h = _create(lib, dtype, np.float32, 16, 0, 0, null_taps=True)
        assert rc == E_INVALID_ARGUMENT and not h.value
        assert "dtype" in _message(lib)
    rc, h = _create(lib, sd.RR32, np.float32, 16, 0, 0, null_taps=True)  # 2. null taps with len > 0
    assert rc == E_INVALID_ARGUMENT and not h.value
    assert "null" in _message(lib)
    rc, h = _create(lib, sd.RC32, np.float32, 0, 0, 0)  # 3. D = 0, ahead of len = 0 and M = 0
    assert rc == E_DECIMATION_LESS_THAN_ONE and not h.value
    assert "DecimationLessThanOne" in _message(lib)
    for D in (1 << 31, (1 << 64) - 1):  # 4. D > 2^31 - 1
        rc, h = _create(lib, sd.CC32, np.complex64, 0, 0, D)
        assert rc == E_INVALID_ARGUMENT and not h.value
        assert "decimation" in _message(lib)
    rc, h = _create(lib, sd.RR64, np.float64, 0, 0, (1 << 31) - 1)  # 5. the interpolator's: len = 0 first
    assert rc == E_COEFFICIENTS_LENGTH_ZERO and not h.value
    assert "CoefficientsLengthZero" in _message(lib)
    rc, h = _create(lib, sd.CC64, np.complex128, 16, 0, 3)  # then M = 0
    assert rc == E_INTERPOLATION_LESS_THAN_ONE and not h.value
    assert "InterpolationLessThanOne" in _message(lib)
    assert lib.sdsp_resamp_create(None, sd.RC32, None, 0, 1, 1, 0) == E_INVALID_ARGUMENT


def test_no_device_fails_loudly():
    import solid_dsp_amd as sd
    lib = sd.lib()
    if sd.device_count() > 0:
        rc, h = _create(lib, sd.RC32, np.float32, 16, 3, 2, device=sd.device_count() + 7)
    else:
        rc, h = _create(lib, sd.RC32, np.float32, 16, 3, 2)
        with pytest.raises(sd.SdspError) as e:
            sd.Resampler(np.ones(16, dtype=np.float32), 3, 2)
        assert e.value.code == E_NO_DEVICE
    assert rc == E_NO_DEVICE and not h.value  # no CPU fallback


def test_null_handle_calls():
    import solid_dsp_amd as sd
    lib = sd.lib()
    assert lib.sdsp_resamp_interpolation(None) == 0
    assert lib.sdsp_resamp_decimation(None) == 0
    assert lib.sdsp_resamp_subfilter_len(None) == 0
    assert lib.sdsp_resamp_output_count(None, 100) == 0
    assert lib.sdsp_resamp_get_algo(None) == -1
    out = C.c_void_p(0xdead)
    sz, k = C.c_size_t(77), C.c_int(0)
    for call in (lambda: lib.sdsp_resamp_set_algo(None, 1), lambda: lib.sdsp_resamp_reset(None),
                 lambda: lib.sdsp_resamp_set_channels(None, 2), lambda: lib.sdsp_resamp_set_tuning(None, 24, 1),
                 lambda: lib.sdsp_resamp_get_phase(None, C.byref(sz)), lambda: lib.sdsp_resamp_set_phase(None, 0),
                 lambda: lib.sdsp_resamp_info(None, C.byref(k), C.byref(sz)),
                 lambda: lib.sdsp_resamp_synchronize(None), lambda: lib.sdsp_resamp_clone(None, C.byref(out)),
                 lambda: lib.sdsp_resamp_execute_block(None, None, 0, None, C.byref(sz)),
                 lambda: lib.sdsp_resamp_execute_block_device(None, None, 0, None, C.byref(sz), None)):
        assert call() == E_INVALID_ARGUMENT
    lib.sdsp_resamp_destroy(None)  # a no-op


# ---------------------------------------------------------------- sdsp_resamp_count
def _count(lib, M, D, c, n):
    no, nxt = C.c_size_t(1 << 40), C.c_size_t(1 << 40)
    rc = lib.sdsp_resamp_count(M, D, c, n, C.byref(no), C.byref(nxt))
    return rc, no.value, nxt.value


def walk(M, D, c, n):
    """the reference decimator's counter over the n * M interpolated samples of a call: it emits
    on counts D - 1, 2D - 1, ... and restarts from 0 after each"""
    emitted = []
    for u in range(n * M):
        if c == D - 1:
            emitted.append(u)
            c = 0
        else:
            c += 1
    return emitted, c


def test_count_is_the_counter_walk():
    import solid_dsp_amd as sd
    lib = sd.lib()
    for M in range(1, 13):
        for D in range(1, 13):
            for n in range(41):
                total = n * M
                for c in range(D):
                    rc, no, nxt = _count(lib, M, D, c, n)
                    # the walk in closed form (checked against walk() itself below): emissions at
                    # u = D - 1 - c, 2D - 1 - c, ...
                    assert rc == 0 and no == (c + total) // D and nxt == (c + total) % D, (M, D, c, n)
    for M, D in ((1, 1), (3, 2), (2, 3), (5, 7), (4, 6), (12, 5), (7, 12)):
        for c in range(D):
            for n in (0, 1, 2, 5, 40):
                u, nxt = walk(M, D, c, n)
                assert _count(lib, M, D, c, n) == (0, len(u), nxt)
                assert u == [(k + 1) * D - 1 - c for k in range(len(u))]  # the definition's u_k


def test_count_chains_over_ragged_calls():
    import solid_dsp_amd as sd
    lib = sd.lib()
    r = np.random.default_rng(3)
    for M in range(1, 13):  # next_phase feeds the next call: the chain is one long call
        for D in range(1, 13):
            c, total, outs = 0, 0, 0
            for n in r.integers(0, 41, size=12):
                rc, no, c = _count(lib, M, D, c, int(n))
                assert rc == 0
                total += int(n)
                outs += no
                assert outs == total * M // D and c == total * M % D
    M, D, c, total, outs = 147, 160, 0, 0, 0
    for n in r.integers(0, 300, size=1000):
        rc, no, c = _count(lib, M, D, c, int(n))
        assert rc == 0 and c < D
        total += int(n)
        outs += no
    assert outs == total * M // D and c == total * M % D


def test_count_limits():
    import solid_dsp_amd as sd
    lib = sd.lib()
    lim = 1 << 63
    for M, D, c in ((1, 1, 0), (3, 2, 1), (147, 160, 159), (1 << 20, 7, 6), ((1 << 31) - 1, (1 << 31) - 1, 5)):
        n = (lim - 1 - c) // M  # the largest n with c + n M < 2^63
        rc, no, nxt = _count(lib, M, D, c, n)
        assert rc == 0 and no == (c + n * M) // D and nxt == (c + n * M) % D, (M, D, c)
        for over in (n + 1, n + 2, (1 << 64) - 1):
            assert c + over * M >= lim
            assert _count(lib, M, D, c, over)[0] == E_INVALID_ARGUMENT, (M, D, c, over)
    assert _count(lib, 1, 1, 0, lim - 1) == (0, lim - 1, 0)
    assert _count(lib, 1, 1, 0, lim)[0] == E_INVALID_ARGUMENT
    assert _count(lib, 0, 2, 0, 5)[0] == E_INVALID_ARGUMENT  # M = 0
    assert _count(lib, 2, 0, 0, 5)[0] == E_INVALID_ARGUMENT  # D = 0
    assert _count(lib, 2, 3, 3, 5)[0] == E_INVALID_ARGUMENT  # phase >= D
    assert lib.sdsp_resamp_count(3, 2, 1, 5, None, None) == 0  # both results are optional


# ---------------------------------------------------------------- what the GPU cases can see
def _rel(y, ref):
    return float(np.linalg.norm(y - ref) / np.linalg.norm(ref))


def test_what_the_inputs_see():
    """On the oracle alone: with white taps and white input, a selection one phase off and a
    reversed tap vector each move the strided output by more than 0.5 rel-RMS (measured: 1.47 to
    1.55 and 1.46), so the GPU cases of tests/test_gpu_resamp.py tell both mistakes from rounding.
    With firdes_kaiser taps the reversed vector moves it by 0.0 (the taps are symmetric), which is
    why every case there uses white taps."""
    M, D, K, n = 5, 7, 4, 700
    r = np.random.default_rng(21)
    h = r.standard_normal(K * M) / np.sqrt(K * M)
    x = r.standard_normal(n)
    z = O.interp(O.RR64, h, M).execute_block(x)
    ref = z[D - 1::D]
    for off in (1, 2, D - 1):  # one phase off, either way
        y = z[(D - 1 + off) % D::D]
        m = min(len(y), len(ref))
        assert _rel(y[:m], ref[:m]) > 0.5, off
    zr = O.interp(O.RR64, h[::-1].copy(), M).execute_block(x)
    assert _rel(zr[D - 1::D], ref) > 0.5
    k = O.firdes_kaiser(K * M, 0.1, 60.0, 0.0)
    zk = O.interp(O.RR64, k, M).execute_block(x)
    zkr = O.interp(O.RR64, k[::-1].copy(), M).execute_block(x)
    assert _rel(zkr[D - 1::D], zk[D - 1::D]) < 1e-12
