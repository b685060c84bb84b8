"""CPU-side checks of the up-converter's C-ABI boundary (sdsp_duc_*, include/sdsp.h): the
symbols are exported, and create refuses bad arguments and a missing device before any device
work.  No compute calls (the library has no CPU path)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "sdsp.h")

E_COEFFICIENTS_LENGTH_ZERO, E_INTERPOLATION_LESS_THAN_ONE = 1, 3
E_INVALID_ARGUMENT, E_NO_DEVICE = 90, 101


def duc_symbols():
    text = open(HDR).read()
    return sorted(set(re.findall(r"SDSP_API\s+[\w\s\*]+?\b(sdsp_duc_\w+)\s*\(", text)))


def test_header_declares_the_duc_family():
    syms = duc_symbols()
    names = ("create", "destroy", "clone", "reset", "set_channels", "set_algo", "get_algo", "set_direction",
             "set_frequency", "adjust_frequency", "set_phase", "adjust_phase", "get_nco_state", "set_nco_state",
             "interpolation", "subfilter_len", "execute_block", "execute_block_device", "synchronize")
    for name in names:
        assert "sdsp_duc_" + name in syms, name
    assert len(syms) == len(names)  # no window get / set: the interpolator handle has none


def test_library_exports_every_duc_symbol():
    import solid_dsp_amd as sd
    out = subprocess.run(["nm", "-D", "--defined-only", sd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sdsp_\w+)", out))
    missing = [s for s in duc_symbols() if s not in exported]
    assert not missing, missing
    lib = sd.lib()  # and the Python loader binds them
    for s in duc_symbols():
        assert hasattr(lib, s)
    assert sd.DUC is sd.duc.DUC


def _create(lib, dtype, coef_dt, len_, M, device=0):
    taps = np.ones(max(len_, 1), dtype=coef_dt)
    h = C.c_void_p(0xdead)  # create must null it on every failure
    rc = lib.sdsp_duc_create(C.byref(h), dtype, taps.ctypes.data_as(C.c_void_p), len_, M, device)
    return rc, h


def _message(lib):
    m = lib.sdsp_last_error()
    return m.decode() if isinstance(m, bytes) else (m or "")


def test_create_refuses_bad_arguments():
    """argument checks come before the device check, so they hold with and without a GPU"""
    import solid_dsp_amd as sd
    lib = sd.lib()
    for dtype, dt in ((sd.RR32, np.float32), (sd.RR64, np.float64)):  # real samples
        rc, h = _create(lib, dtype, dt, 16, 4)
        assert rc == E_INVALID_ARGUMENT and not h.value, (dtype, rc)
        assert "complex" in _message(lib)
    for dtype in (-1, 6):
        rc, h = _create(lib, dtype, np.float32, 16, 4)
        assert rc == E_INVALID_ARGUMENT and not h.value
        assert "complex" in _message(lib)
    rc, h = _create(lib, sd.RC32, np.float32, 0, 4)  # zero taps: the interpolator's own code
    assert rc == E_COEFFICIENTS_LENGTH_ZERO and not h.value
    assert "CoefficientsLengthZero" in _message(lib)
    rc, h = _create(lib, sd.CC64, np.complex128, 16, 0)  # M = 0
    assert rc == E_INTERPOLATION_LESS_THAN_ONE and not h.value
    assert "InterpolationLessThanOne" in _message(lib)
    assert lib.sdsp_duc_create(None, sd.RC32, None, 0, 1, 0) == E_INVALID_ARGUMENT


def test_no_device_fails_loudly():
    import solid_dsp_amd as sd
    lib = sd.lib()
    if sd.device_count() > 0:
        rc, h = _create(lib, sd.RC32, np.float32, 16, 4, device=sd.device_count() + 7)
    else:
        rc, h = _create(lib, sd.RC32, np.float32, 16, 4)
        with pytest.raises(sd.SdspError) as e:
            sd.DUC(np.ones(16, dtype=np.float32), 4, sample_dtype=np.complex64)
        assert e.value.code == E_NO_DEVICE
    assert rc == E_NO_DEVICE and not h.value  # no CPU fallback


def test_null_handle_calls():
    import solid_dsp_amd as sd
    lib = sd.lib()
    assert lib.sdsp_duc_interpolation(None) == 0
    assert lib.sdsp_duc_subfilter_len(None) == 0
    assert lib.sdsp_duc_get_algo(None) == -1
    out = C.c_void_p(0xdead)
    for call in (lambda: lib.sdsp_duc_set_algo(None, 1), lambda: lib.sdsp_duc_set_direction(None, 0),
                 lambda: lib.sdsp_duc_set_frequency(None, 0.1), lambda: lib.sdsp_duc_adjust_frequency(None, 0.1),
                 lambda: lib.sdsp_duc_set_phase(None, 0.1), lambda: lib.sdsp_duc_adjust_phase(None, 0.1),
                 lambda: lib.sdsp_duc_reset(None), lambda: lib.sdsp_duc_set_channels(None, 2),
                 lambda: lib.sdsp_duc_get_nco_state(None, None, None),
                 lambda: lib.sdsp_duc_set_nco_state(None, 1, 2), lambda: lib.sdsp_duc_synchronize(None),
                 lambda: lib.sdsp_duc_clone(None, C.byref(out)),
                 lambda: lib.sdsp_duc_execute_block(None, None, 0, None),
                 lambda: lib.sdsp_duc_execute_block_device(None, None, 0, None, None)):
        assert call() == E_INVALID_ARGUMENT
    lib.sdsp_duc_destroy(None)  # a no-op
