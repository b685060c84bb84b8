"""CPU-side checks of the spectrometer's C-ABI boundary (sdsp_spec_*, include/sdsp.h) and of the numpy
restatements its GPU tests stand on (tests/spec_cases.py): the symbols are exported and bound,
sdsp_spec_count is the frame walk, create refuses bad arguments in its documented order before any device
work, the restatements agree with each other and with closed forms, f32 arithmetic alone stays inside
half the GPU tolerance, and the inputs of tests/test_gpu_spec.py can see the summation orders they are
there to tell apart.  No compute calls (the library has no CPU path)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spec_cases import (AS, BLOCKS, C64, C128, DEFINITION, F32, F64, FRAMES, MAX_A, SETTINGS, SHAPES, count, power,
                        slide_fits, spec_f32, spec_fold, spec_plan, spec_ref, white_input)
from oschan_cases import oschan_f32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "sdsp.h")

E_COEFFICIENTS_LENGTH_ZERO, E_NOT_ENOUGH_FILTERS = 1, 4
E_INVALID_ARGUMENT, E_UNSUPPORTED, E_NO_DEVICE = 90, 91, 101
NAMES = ("create", "destroy", "set_streams", "set_tuning", "reset", "set_scale", "channels", "decimation",
         "subfilter_len", "integration", "phase", "filled", "execute_block", "execute_block_device", "info",
         "synchronize", "count")


def spec_symbols():
    text = open(HDR).read()
    return sorted(set(re.findall(r"SDSP_API\s+[\w\s\*]+?\b(sdsp_spec_\w+)\s*\(", text)))


def test_header_declares_the_family():
    assert len(NAMES) == 17
    assert spec_symbols() == sorted("sdsp_spec_" + n for n in NAMES)
    text = open(HDR).read()
    assert re.search(r"SDSP_TUNE_SPEC_KERNEL\s*=\s*31\b", text)
    assert re.search(r"SDSP_TUNE_SPEC_SUBBLOCKS\s*=\s*32\b", text)
    for getter in ("channels", "decimation", "subfilter_len", "integration", "phase", "filled"):
        assert re.search(rf"SDSP_API\s+size_t\s+sdsp_spec_{getter}\s*\(\s*const\s+sdsp_spec\s*\*", text), getter


def test_library_exports_and_python_binds_every_symbol():
    import solid_dsp_amd as sd
    out = subprocess.run(["nm", "-D", "--defined-only", sd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sdsp_\w+)", out))
    missing = [s for s in spec_symbols() if s not in exported]
    assert not missing, missing
    lib = sd.lib()
    for s in spec_symbols():
        assert getattr(lib, s).argtypes is not None, s  # declared by _lib, not merely found
    assert sd.Spectrometer is sd.spectrometer.Spectrometer
    assert (sd._lib.TUNE_SPEC_KERNEL, sd._lib.TUNE_SPEC_SUBBLOCKS) == (31, 32)
    assert sd.Spectrometer.KERNELS == {1: "per_frame", 2: "sliding"}


# ---------------------------------------------------------------- sdsp_spec_count
def _filled_classes(A):
    return sorted({f for f in (0, 1, 31, 32, 33, A // 2, A - 33, A - 32, A - 1) if 0 <= f < A})


@pytest.mark.parametrize("A", [1, 31, 32, 33, MAX_A])
@pytest.mark.parametrize("D", [1, 3, 512])
def test_count_is_the_frame_walk(D, A):
    import solid_dsp_amd as sd
    checked = 0
    for filled in _filled_classes(A):
        left = A - filled
        for frames in sorted({0, 1, left - 1, left, left + 1, left + A, 2 * A + 3, 3 * A} - {-1}):
            want = count(D, A, filled, frames * D)
            assert sd.Spectrometer.count(D, A, filled, frames * D) == want, (D, A, filled, frames)
            checked += 1
    assert checked >= 5


def test_count_refusals_and_optional_results():
    import solid_dsp_amd as sd
    lib = sd.lib()
    sp, nf = C.c_size_t(77), C.c_size_t(77)
    for D, A, filled, n in ((0, 4, 0, 8), (2, 0, 0, 8), (2, MAX_A + 1, 0, 8), (2, 4, 4, 8), (2, 4, 9, 8),
                            (3, 4, 0, 8), (512, 4, 0, 511)):
        assert lib.sdsp_spec_count(D, A, filled, n, C.byref(sp), C.byref(nf)) == E_INVALID_ARGUMENT, (D, A, filled, n)
        assert (sp.value, nf.value) == (77, 77)  # a refusal writes nothing
        with pytest.raises(sd.SdspError) as e:
            sd.Spectrometer.count(D, A, filled, n)
        assert e.value.code == E_INVALID_ARGUMENT
    assert lib.sdsp_spec_count(2, 4, 3, 10, None, None) == 0
    assert lib.sdsp_spec_count(2, 4, 3, 10, C.byref(sp), None) == 0 and sp.value == 2
    assert lib.sdsp_spec_count(2, 4, 3, 10, None, C.byref(nf)) == 0 and nf.value == 0
    assert sd.Spectrometer.count(2, MAX_A, MAX_A - 1, 2) == (1, 0)


# ---------------------------------------------------------------- create
def _create(lib, dtype, len_, M, D, A, device=0, null_taps=False, coef_dt=np.float32):
    taps = np.ones(max(len_, 1), dtype=coef_dt)
    h = C.c_void_p(0xdead)  # create must null it on every failure
    p = None if null_taps else taps.ctypes.data_as(C.c_void_p)
    rc = lib.sdsp_spec_create(C.byref(h), dtype, p, len_, M, D, A, device)
    return rc, h


def _message(lib):
    m = lib.sdsp_last_error()
    return m.decode() if isinstance(m, bytes) else (m or "")


def test_create_refuses_bad_arguments_in_order():
    """every argument check comes before the device check, so this holds with and without a GPU; each
    call breaks one more rule than the check it expects to fire, so the order shows"""
    import solid_dsp_amd as sd
    lib = sd.lib()
    assert lib.sdsp_spec_create(None, -1, None, 16, 0, 0, 0, 0) == E_INVALID_ARGUMENT  # 1. null out
    for dtype in (-1, sd.RR32, sd.CC32, sd.RR64, sd.CC64, 6):  # 2. dtype, ahead of null taps and channels = 0
        rc, h = _create(lib, dtype, 16, 0, 0, 0, null_taps=True)
        assert rc == E_UNSUPPORTED and not h.value, dtype
        assert "SDSP_RC32" in _message(lib)
    rc, h = _create(lib, sd.RC32, 16, 0, 0, 0, null_taps=True)  # 3. null taps with len > 0
    assert rc == E_INVALID_ARGUMENT and not h.value and "null" in _message(lib)
    rc, h = _create(lib, sd.RC32, 0, 0, 0, 0)  # 4. channels = 0, ahead of len = 0
    assert rc == E_NOT_ENOUGH_FILTERS and not h.value and "NotEnoughFilters" in _message(lib)
    rc, h = _create(lib, sd.RC64, 0, 3, 0, 0, null_taps=True, coef_dt=np.float64)  # 5. len = 0
    assert rc == E_COEFFICIENTS_LENGTH_ZERO and not h.value and "CoefficientsLengthZero" in _message(lib)
    for M in (1, 2, 3, 12, 1000, 8192, 1 << 20):  # 6. not a power of two in [4, 4096], ahead of decimation = 0
        rc, h = _create(lib, sd.RC32, 1, M, 0, 0)
        assert rc == E_UNSUPPORTED and not h.value, M
        assert "power of two" in _message(lib)
    for M, D in ((4, 0), (4, 5), (64, 65), (4096, 1 << 40)):  # 7. decimation, ahead of integration = 0
        rc, h = _create(lib, sd.RC32, M - 1, M, D, 0)
        assert rc == E_UNSUPPORTED and not h.value, (M, D)
        assert "decimation" in _message(lib)
    for A in (0, MAX_A + 1, 1 << 40):  # 8. integration outside [1, 32768], ahead of len < channels
        rc, h = _create(lib, sd.RC32, 63, 64, 48, A)
        assert rc == E_UNSUPPORTED and not h.value, A
        assert "integration" in _message(lib)
    for M, n, D, A in ((4, 3, 4, 1), (64, 63, 1, MAX_A), (4096, 4095, 3000, 33)):  # 9. len < channels
        rc, h = _create(lib, sd.RC32, n, M, D, A)
        assert rc == E_INVALID_ARGUMENT and not h.value, (M, n)
        assert "fewer taps" in _message(lib)


def test_no_device_fails_loudly():
    import solid_dsp_amd as sd
    lib = sd.lib()
    if sd.device_count() > 0:
        rc, h = _create(lib, sd.RC32, 16, 8, 6, 5, device=sd.device_count() + 7)
    else:
        rc, h = _create(lib, sd.RC32, 16, 8, 6, 5)
        with pytest.raises(sd.SdspError) as e:
            sd.Spectrometer(np.ones(16, dtype=np.float32), 8, 6, 5)
        assert e.value.code == E_NO_DEVICE
    assert rc == E_NO_DEVICE and not h.value  # no CPU fallback


def test_null_handle_calls():
    import solid_dsp_amd as sd
    lib = sd.lib()
    for getter in (lib.sdsp_spec_channels, lib.sdsp_spec_decimation, lib.sdsp_spec_subfilter_len,
                   lib.sdsp_spec_integration, lib.sdsp_spec_phase, lib.sdsp_spec_filled):
        assert getter(None) == 0
    sz, k = C.c_size_t(77), C.c_int(0)
    for call in (lambda: lib.sdsp_spec_reset(None), lambda: lib.sdsp_spec_set_streams(None, 2),
                 lambda: lib.sdsp_spec_set_tuning(None, 31, 1), lambda: lib.sdsp_spec_set_tuning(None, 32, 8),
                 lambda: lib.sdsp_spec_set_scale(None, 0.5),
                 lambda: lib.sdsp_spec_info(None, C.byref(k), C.byref(sz)),
                 lambda: lib.sdsp_spec_synchronize(None),
                 lambda: lib.sdsp_spec_execute_block(None, None, 0, None, C.byref(sz)),
                 lambda: lib.sdsp_spec_execute_block_device(None, None, 0, None, C.byref(sz), None)):
        assert call() == E_INVALID_ARGUMENT
    lib.sdsp_spec_destroy(None)  # a no-op


# ---------------------------------------------------------------- the case tables
def test_the_grid_covers_every_class():
    assert len(SHAPES) == 50 and len(set(SHAPES)) == 50
    for prec in (C64, C128):
        for M in (4, 64, 256, 1024, 4096):
            mine = [(K, D) for m, K, D, _, p in SHAPES if m == M and p == prec]
            assert {K for K, _ in mine} == {1, 3, 8, 12}
            assert {1, M // 2, 3 * M // 4, M} <= {D for _, D in mine}
            assert any(M % D for _, D in mine)
    for A in AS:  # every A meets the per-frame kernel (it runs every shape), the sliding kernel and both precisions
        assert {p for *_, a, p in SHAPES if a == A} == {C64, C128}, A
        assert any(slide_fits(M, K, D, p) for M, K, D, a, p in SHAPES if a == A), A
    # K = 12 is a depth without a register instance; the settings reach runs of one and of several sub-blocks
    assert any(K == 12 and slide_fits(M, K, D, p) for M, K, D, _, p in SHAPES)
    assert {k for k, _ in SETTINGS} == {1, 2} and {0, 1, 3} <= {r for _, r in SETTINGS}
    assert sum(BLOCKS) == FRAMES
    kernels = {spec_plan(M, K, D, A, p, 2, 0)[0] for M, K, D, A, p in DEFINITION}
    assert kernels == {1, 2} and {p for *_, p in DEFINITION} == {C64, C128}


def test_plan_restatement():
    assert spec_plan(64, 8, 32, 32, C64) == (2, 2)       # fill 15 frames: two sub-blocks of 32 reach 60
    assert spec_plan(64, 8, 16, 32, C64) == (2, 4)       # fill 31 frames
    assert spec_plan(64, 8, 32, 5, C64) == (2, 12)       # sub-blocks of 5 frames
    assert spec_plan(64, 8, 64, 1024, C64) == (2, 1)     # fill 7 frames
    assert spec_plan(64, 1, 64, 1, C64) == (2, 1)        # no fill at all: at least one
    assert spec_plan(64, 8, 1, 100, C64) == (2, 64)      # fill 511 frames
    assert spec_plan(256, 8, 128, 32, C64) == (2, 2)     # 25 KiB
    assert spec_plan(1024, 1, 1024, 32, C64) == (2, 1)   # 40 KiB to the byte
    assert spec_plan(1024, 1, 1024, 32, C128) == (1, 1)
    assert spec_plan(256, 1, 128, 32, C64) == (1, 1)     # the measured exception
    assert spec_plan(256, 1, 128, 32, C64, 2) == (2, 1)
    assert spec_plan(1024, 8, 512, 32, C64) == (1, 1)    # 92 KiB: automatic is the per-frame kernel
    assert spec_plan(1024, 8, 512, 32, C64, 2) == (2, 2)
    assert spec_plan(1024, 8, 512, 32, C64, 2, 7) == (2, 7)
    assert spec_plan(1024, 8, 512, 32, C64, 1, 7) == (1, 7)
    assert spec_plan(4096, 3, 4096, 32, C64, 2) == (1, 1)  # does not fit 128 KiB


# ---------------------------------------------------------------- the restatements
@pytest.mark.parametrize("A", [1, 5, 33, 100])
def test_split_fold_is_the_whole_fold(A):
    """spec_fold call by call with the state carried equals one call, bit for bit"""
    p = np.random.default_rng(7).random((2, FRAMES, 8)).astype(F32)
    whole, wf, wsub, wtot = spec_fold(p, A, 0, None, None, 0.3, F32)
    assert whole.shape == (2, FRAMES // A, 8) and wf == FRAMES % A
    state, out, a = (0, None, None), [], 0
    for nb in BLOCKS:
        sp, *state = spec_fold(p[:, a:a + nb], A, *state, 0.3, F32)
        out.append(sp)
        a += nb
    assert np.array_equal(np.concatenate(out, axis=1), whole)
    assert state[0] == wf and np.array_equal(state[1], wsub) and np.array_equal(state[2], wtot)


@pytest.mark.parametrize("A", [1, 31, 32, 33, 100])
def test_fold_in_f64_is_a_plain_sum(A):
    p = np.random.default_rng(11).random((FRAMES, 16))
    got = spec_fold(p, A, 0, None, None, 0.25, F64)[0]
    J = FRAMES // A
    want = p[:J * A].reshape(J, A, 16).sum(axis=1) * 0.25
    assert got.shape == want.shape
    assert np.max(np.abs(got - want) / want) <= 1e-14


@pytest.mark.parametrize("M", [64, 1024])
@pytest.mark.parametrize("A", [5, 100])
def test_dc_closed_form(M, A):
    """an all-ones window of M points (K = 1), D = M and x = 0.5: every frame's DC bin is M/2 and every
    other bin 0, so P[0] = A M^2 / 4 and the rest 0, exactly, in f32 and in the definition"""
    h, x = np.ones(M, F32), np.full(M * FRAMES, 0.5, C64)
    for P in (spec_f32(h, M, M, A, x), spec_ref(h, M, M, A, x)):
        assert P.shape == (FRAMES // A, M)
        assert np.all(P[:, 0] == A * M * M / 4) and not P[:, 1:].any()


@pytest.mark.parametrize("M,K,D,A", [(64, 8, 48, 100), (1024, 3, 1000, 33), (4096, 1, 2048, 65)])
def test_f32_arithmetic_alone_stays_inside(M, K, D, A):
    """f32 branch sums, a single-precision FFT and the f32 fold on the CPU, white taps and a white stream,
    230 frames: every spectrum within 5e-7 of the definition, half the GPU limit"""
    h, x = white_input(M, K, D)
    got, ref = spec_f32(h, M, D, A, x[0]).astype(F64), spec_ref(h, M, D, A, x[0])
    rel = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
    print(f"f32 on the CPU M={M} K={K} D={D} A={A}: worst spectrum {rel.max():.3e} (limit 5e-07)")
    assert rel.max() <= 5e-7


@pytest.mark.parametrize("M,K,D", [(64, 8, 48), (256, 1, 128)])
def test_what_the_inputs_see(M, K, D):
    """on the white inputs of the GPU tests three other summation orders each change bits of the
    spectra: sub-blocks cut every 31 frames, cuts that ignore the restart at the integration boundary,
    and every frame added straight onto the integration's sum.  Blind spots: a cut of 31 is invisible
    up to A = 31, the missing restart wherever 32 divides A, and the other nesting up to A = 33"""
    h, x = white_input(M, K, D)
    p = power(oschan_f32(h, M, D, x[0]), F32)
    for A in (33, 65, 100):
        good = spec_fold(p, A, 0, None, None, 1.0, F32)[0]
        for what, bad in (("cut at 31", spec_fold(p, A, 0, None, None, 1.0, F32, cut=31)[0]),
                          ("no restart", spec_fold(p, A, 0, None, None, 1.0, F32, restart=False)[0]),
                          ("other nesting", spec_fold(p, A, 0, None, None, 1.0, F32, flat=True)[0])):
            if A == 33 and what == "other nesting":  # (s_0 + p[32] either way)
                assert np.array_equal(good, bad)
                continue
            changed = int(np.count_nonzero(good != bad))
            print(f"M={M} K={K} D={D} A={A} {what}: {changed} of {good.size} values differ")
            assert changed > good.size // 20, (what, A, changed)
            assert np.max(np.abs(good - bad) / good) < 1e-5  # (an order of summation, not another sum)
    for A in (5, 31):
        assert np.array_equal(spec_fold(p, A, 0, None, None, 1.0, F32, cut=31)[0],
                              spec_fold(p, A, 0, None, None, 1.0, F32)[0])
    assert np.array_equal(spec_fold(p, 64, 0, None, None, 1.0, F32, restart=False)[0],
                          spec_fold(p, 64, 0, None, None, 1.0, F32)[0])
