"""CPU-side checks of the arbitrary-rate resampler's C-ABI boundary (sdsp_arb_*, include/sdsp.h):
the symbols are exported, create refuses bad arguments in its documented order and a missing
device before any device work, sdsp_arb_count (the index arithmetic every call runs on) equals a
brute-force walk of the time accumulator, sdsp_arb_step_from_rate rounds as documented, and the
oracle alone shows what the GPU cases of tests/test_gpu_arb.py can see.  No compute calls (the
library has no CPU path)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import arb_cases as A
import oracle_lib as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "sdsp.h")

E_COEFFICIENTS_LENGTH_ZERO, E_INTERPOLATION_LESS_THAN_ONE = 1, 3
E_INVALID_ARGUMENT, E_NO_DEVICE = 90, 101
GOOD_STEP = 1 << 32


def arb_symbols():
    text = open(HDR).read()
    return sorted(set(re.findall(r"SDSP_API\s+[\w\s\*]+?\b(sdsp_arb_\w+)\s*\(", text)))


def test_header_declares_the_arb_family():
    syms = arb_symbols()
    names = ("create", "destroy", "clone", "reset", "set_channels", "set_algo", "get_algo", "set_tuning", "filters",
             "subfilter_len", "get_step", "set_step", "get_time", "set_time", "output_count", "execute_block",
             "execute_block_device", "info", "synchronize", "count", "step_from_rate")
    for name in names:
        assert "sdsp_arb_" + name in syms, name
    assert len(syms) == len(names)  # no per-sample entry point, scale or window get / set
    assert re.search(r"SDSP_TUNE_ARB_KERNEL\s*=\s*29\b", open(HDR).read())


def test_library_exports_every_arb_symbol():
    import solid_dsp_amd as sd
    out = subprocess.run(["nm", "-D", "--defined-only", sd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sdsp_\w+)", out))
    missing = [s for s in arb_symbols() if s not in exported]
    assert arb_symbols() and not missing, missing
    lib = sd.lib()  # and the Python loader binds them
    for s in arb_symbols():
        assert hasattr(lib, s)
    assert sd.ArbResampler is sd.arb.ArbResampler
    assert sd._lib.TUNE_ARB_KERNEL == 29


def _create(lib, dtype, coef_dt, len_, filters, step, device=0, null_taps=False):
    taps = np.ones(max(len_, 1), dtype=coef_dt)
    h = C.c_void_p(0xdead)  # create must null it on every failure
    p = None if null_taps else taps.ctypes.data_as(C.c_void_p)
    rc = lib.sdsp_arb_create(C.byref(h), dtype, p, len_, filters, step, device)
    return rc, h


def _message(lib):
    m = lib.sdsp_last_error()
    return m.decode() if isinstance(m, bytes) else (m or "")


def test_create_refuses_bad_arguments_in_order():
    """every argument check comes before the device check, so this holds with and without a GPU;
    each call breaks one more rule than the check it expects to fire, so the order shows"""
    import solid_dsp_amd as sd
    lib = sd.lib()
    for dtype in (-1, 6):  # 1. dtype, ahead of null taps, the step, filters, len = 0
        rc, h = _create(lib, dtype, np.float32, 16, 1 << 31, 0, null_taps=True)
        assert rc == E_INVALID_ARGUMENT and not h.value
        assert "dtype" in _message(lib)
    rc, h = _create(lib, sd.RR32, np.float32, 16, 1 << 31, 0, null_taps=True)  # 2. null taps with len > 0
    assert rc == E_INVALID_ARGUMENT and not h.value
    assert "null" in _message(lib)
    for step in (0, (1 << 16) - 1, (1 << 48) + 1, (1 << 64) - 1):  # 3. the step, ahead of filters and len = 0
        rc, h = _create(lib, sd.RC32, np.float32, 0, 1 << 31, step)
        assert rc == E_INVALID_ARGUMENT and not h.value, step
        assert "step" in _message(lib)
    for filters in (1 << 31, (1 << 64) - 1):  # 4. filters > 2^31 - 1, ahead of len = 0
        for step in (1 << 16, 1 << 48):  # (both ends of the step's range are inside it)
            rc, h = _create(lib, sd.CC32, np.complex64, 0, filters, step)
            assert rc == E_INVALID_ARGUMENT and not h.value
            assert "filters" in _message(lib)
    rc, h = _create(lib, sd.RR64, np.float64, 0, 0, GOOD_STEP)  # 5. the interpolator's: len = 0 first
    assert rc == E_COEFFICIENTS_LENGTH_ZERO and not h.value
    assert "CoefficientsLengthZero" in _message(lib)
    rc, h = _create(lib, sd.CC64, np.complex128, 16, 0, GOOD_STEP)  # then filters = 0
    assert rc == E_INTERPOLATION_LESS_THAN_ONE and not h.value
    assert "InterpolationLessThanOne" in _message(lib)
    assert lib.sdsp_arb_create(None, sd.RC32, None, 0, 1, GOOD_STEP, 0) == E_INVALID_ARGUMENT


def test_no_device_fails_loudly():
    import solid_dsp_amd as sd
    lib = sd.lib()
    if sd.device_count() > 0:
        rc, h = _create(lib, sd.RC32, np.float32, 16, 4, GOOD_STEP, device=sd.device_count() + 7)
    else:
        rc, h = _create(lib, sd.RC32, np.float32, 16, 4, GOOD_STEP)
        with pytest.raises(sd.SdspError) as e:
            sd.ArbResampler(np.ones(16, dtype=np.float32), 4, rate=0.75)
        assert e.value.code == E_NO_DEVICE
    assert rc == E_NO_DEVICE and not h.value  # no CPU fallback


def test_the_class_wants_exactly_one_of_rate_and_step():
    import solid_dsp_amd as sd
    taps = np.ones(16, dtype=np.float32)
    with pytest.raises(ValueError):
        sd.ArbResampler(taps, 4)
    with pytest.raises(ValueError):
        sd.ArbResampler(taps, 4, rate=1.0, step=GOOD_STEP)
    with pytest.raises(sd.SdspError) as e:  # the rate's step leaves the range before any handle is made
        sd.ArbResampler(taps, 4, rate=2.0 ** 17)
    assert e.value.code == E_INVALID_ARGUMENT


def test_null_handle_calls():
    import solid_dsp_amd as sd
    lib = sd.lib()
    assert lib.sdsp_arb_filters(None) == 0
    assert lib.sdsp_arb_subfilter_len(None) == 0
    assert lib.sdsp_arb_output_count(None, 100) == 0
    assert lib.sdsp_arb_get_algo(None) == -1
    out = C.c_void_p(0xdead)
    sz, k, u = C.c_size_t(77), C.c_int(0), C.c_uint64(5)
    for call in (lambda: lib.sdsp_arb_set_algo(None, 1), lambda: lib.sdsp_arb_reset(None),
                 lambda: lib.sdsp_arb_set_channels(None, 2), lambda: lib.sdsp_arb_set_tuning(None, 29, 1),
                 lambda: lib.sdsp_arb_get_step(None, C.byref(u)), lambda: lib.sdsp_arb_set_step(None, GOOD_STEP),
                 lambda: lib.sdsp_arb_get_time(None, C.byref(u)), lambda: lib.sdsp_arb_set_time(None, 0),
                 lambda: lib.sdsp_arb_info(None, C.byref(k), C.byref(sz)),
                 lambda: lib.sdsp_arb_synchronize(None), lambda: lib.sdsp_arb_clone(None, C.byref(out)),
                 lambda: lib.sdsp_arb_execute_block(None, None, 0, None, C.byref(sz)),
                 lambda: lib.sdsp_arb_execute_block_device(None, None, 0, None, C.byref(sz), None)):
        assert call() == E_INVALID_ARGUMENT
    assert u.value == 5  # nothing written
    lib.sdsp_arb_destroy(None)  # a no-op


# ---------------------------------------------------------------- sdsp_arb_count
def _count(lib, step, t, n):
    no, nxt = C.c_size_t(1 << 40), C.c_uint64(1 << 40)
    rc = lib.sdsp_arb_count(step, t, n, C.byref(no), C.byref(nxt))
    return rc, no.value, nxt.value


def test_count_is_the_accumulator_walk():
    """random step in [2^16, 2^36) (its exponent uniform, so short and long walks both occur), t in
    [0, 2^35), n in [0, 40), walks under 2 * 10^5 steps: the C function, the closed form and the
    brute-force walk agree on 3000 triples"""
    import solid_dsp_amd as sd
    lib = sd.lib()
    r = np.random.default_rng(29)
    done = zero_out = 0
    while done < 3000:
        e = int(r.integers(16, 36))
        step = int(r.integers(1 << e, 1 << (e + 1)))
        t = int(r.integers(0, 1 << 35))
        n = int(r.integers(0, 40))
        if n * A.ONE // step >= 200000:
            continue
        want = A.walk(step, t, n)
        assert A.count(step, t, n) == want, (step, t, n)
        assert _count(lib, step, t, n) == (0,) + want, (step, t, n)
        done += 1
        zero_out += want[0] == 0
    assert 0 < zero_out < done  # calls that emit nothing are among them
    for step, t, n in ((A.ONE, 0, 5), (A.ONE, 1, 5), (A.ONE + 1, 0, 5), (A.ONE - 1, 0, 5), (3 * A.ONE, 5 * A.ONE, 5),
                       (3 * A.ONE, 5 * A.ONE - 1, 5), (1 << 16, 0, 1), (1 << 48, 0, 39)):
        assert _count(lib, step, t, n) == (0,) + A.walk(step, t, n), (step, t, n)
    assert _count(lib, A.ONE, 0, 5) == (0, 5, 0) and _count(lib, A.ONE, 1, 5) == (0, 5, 1)


def test_count_chains_over_ragged_calls():
    """next_t feeds the next call: a chain of ragged calls, some with n = 0 and some that emit
    nothing, is one long call"""
    import solid_dsp_amd as sd
    lib = sd.lib()
    r = np.random.default_rng(3)
    for step in [A.step_of(rate) for rate in A.RATES] + [A.ONE, A.ONE + 1, 17 * A.ONE + 12345, 1 << 40, 1 << 20]:
        t, total, outs, empty, silent = 0, 0, 0, 0, 0
        for n in r.choice([0, 0, 1, 2, 3, 7, 8, 9, 40, 300], size=200):
            rc, no, t = _count(lib, step, t, int(n))
            assert rc == 0
            total += int(n)
            outs += no
            empty += n == 0
            silent += n > 0 and no == 0
            assert (outs, t) == A.count(step, 0, total), (step, total)
        assert empty > 0 and (silent > 0 or step <= A.ONE + 1)
        assert _count(lib, step, 0, total) == (0, outs, t)


def test_count_limits():
    import solid_dsp_amd as sd
    lib = sd.lib()
    n = (1 << 31) - 1
    assert _count(lib, 1 << 16, 0, n) == (0, n << 16, 0)  # the largest call at the smallest step
    assert _count(lib, 1 << 16, 0, 1 << 31)[0] == E_INVALID_ARGUMENT
    assert _count(lib, 1 << 16, 0, (1 << 64) - 1)[0] == E_INVALID_ARGUMENT
    t = (1 << 63) - 1
    assert _count(lib, 1 << 48, t, n) == (0,) + A.count(1 << 48, t, n)
    assert _count(lib, 1 << 48, 1 << 63, 5)[0] == E_INVALID_ARGUMENT  # t >= 2^63
    for step in (0, (1 << 16) - 1, (1 << 48) + 1):
        assert _count(lib, step, 0, 5)[0] == E_INVALID_ARGUMENT
    assert lib.sdsp_arb_count(A.ONE, 0, 5, None, None) == 0  # both results are optional


def test_step_from_rate():
    import solid_dsp_amd as sd
    lib = sd.lib()
    for rate in (1.0, 0.5, 3.0, 0.91875123, 2.0 ** 16, 2.0 ** -16):
        s = C.c_uint64(0)
        assert lib.sdsp_arb_step_from_rate(rate, C.byref(s)) == 0
        assert s.value == A.step_of(rate) == sd.arb.step_from_rate(rate)
        assert abs(s.value - A.ONE / rate) <= 0.5  # 2^32 / rate, rounded to nearest
        assert A.STEP_MIN <= s.value <= A.STEP_MAX
    assert sd.arb.step_from_rate(1.0) == A.ONE and sd.arb.step_from_rate(0.5) == 2 * A.ONE
    assert sd.arb.step_from_rate(2.0 ** 16) == 1 << 16 and sd.arb.step_from_rate(2.0 ** -16) == 1 << 48
    assert sd.arb.step_from_rate(3.0) == (A.ONE + 1) // 3
    for rate in (0.0, -1.0, -0.0, math.nan, math.inf, -math.inf, 2.0 ** 17, 2.0 ** -17):
        s = C.c_uint64(7)
        assert lib.sdsp_arb_step_from_rate(rate, C.byref(s)) == E_INVALID_ARGUMENT, rate
        assert s.value == 7
    assert lib.sdsp_arb_step_from_rate(1.0, None) == E_INVALID_ARGUMENT
    assert sd.arb.count(A.ONE + 1, 3, 40) == A.count(A.ONE + 1, 3, 40)


# ---------------------------------------------------------------- what the GPU cases can see
def _rel(y, ref):
    return float(np.linalg.norm(y - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("P,K", [(32, 8), (64, 16), (7, 4)])
def test_what_the_inputs_see(P, K):
    """On the oracle alone: with white taps and white input, a selection one interpolated sample
    early or late, 1 - mu in place of mu and a reversed tap vector each move the output by more
    than 0.5 rel-RMS at every rate of tests/test_gpu_arb.py (a numpy model gave 0.88 to 1.55), so
    those cases tell each mistake from rounding."""
    import solid_dsp_amd as sd
    n = 1200
    r = np.random.default_rng(21)
    h = r.standard_normal(K * P) / np.sqrt(K * P)
    x = r.standard_normal(n)
    z = O.interp(O.RR64, h, P).execute_block(x)
    zr = O.interp(O.RR64, h[::-1].copy(), P).execute_block(x)
    for rate in A.RATES:
        step = sd.arb.step_from_rate(rate)  # the library's own step and count for the rate
        ref, nxt = A.model(z, 0.0, step, 0, n, P)
        assert step == A.step_of(rate) and (len(ref), nxt) == sd.arb.count(step, 0, n)
        u, m = A.select(step, 0, len(ref), P)
        keep = u >= 1  # (an early a of the stream's first sample would be z(-2))
        assert _rel(A.lerp(z, 0.0, u[keep] - 1, m[keep]), ref[keep]) > 0.5, rate
        keep = u + 1 < len(z)
        assert _rel(A.lerp(z, 0.0, u[keep] + 1, m[keep]), ref[keep]) > 0.5, rate
        assert _rel(A.model(z, 0.0, step, 0, n, P, flip_mu=True)[0], ref) > 0.5, rate
        assert _rel(A.model(zr, 0.0, step, 0, n, P)[0], ref) > 0.5, rate
