"""CPU-side checks of the down-converter's C-ABI boundary (sdsp_ddc_*, include/sdsp.h): the
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

E_INVALID_ARGUMENT, E_NO_DEVICE = 90, 101


def ddc_symbols():
    text = open(HDR).read()
    return sorted(set(re.findall(r"SDSP_API\s+[\w\s\*]+?\b(sdsp_ddc_\w+)\s*\(", text)))


def test_header_declares_the_ddc_family():
    syms = ddc_symbols()
    for name in ("create", "destroy", "clone", "reset", "set_channels", "set_algo", "set_direction", "set_frequency",
                 "adjust_frequency", "set_phase", "adjust_phase", "get_nco_state", "set_nco_state", "output_count",
                 "execute_block", "execute_block_device", "get_state", "set_state", "set_tuning", "synchronize"):
        assert "sdsp_ddc_" + name in syms, name


def test_library_exports_every_ddc_symbol():
    import solid_dsp_amd as sd
    out = subprocess.run(["nm", "-D", "--defined-only", sd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sdsp_\w+)", out))
    missing = [s for s in ddc_symbols() if s not in exported]
    assert not missing, missing
    lib = sd.lib()  # and the Python loader binds them
    for s in ddc_symbols():
        assert hasattr(lib, s)


def _create(lib, dtype, coef_dt, len_, M, device=0):
    taps = np.ones(max(len_, 1), dtype=coef_dt)
    scale = np.ones(1, dtype=coef_dt)
    h = C.c_void_p(0xdead)  # create must null it on every failure
    rc = lib.sdsp_ddc_create(C.byref(h), dtype, taps.ctypes.data_as(C.c_void_p), len_,
                             scale.ctypes.data_as(C.c_void_p), M, device)
    return rc, h


def test_create_refuses_bad_arguments():
    """argument checks come before the device check, so they hold with and without a GPU"""
    import solid_dsp_amd as sd
    lib = sd.lib()
    for dtype, dt in ((sd.RR32, np.float32), (sd.RR64, np.float64)):  # real samples: a later change
        rc, h = _create(lib, dtype, dt, 16, 4)
        assert rc == E_INVALID_ARGUMENT and not h.value, (dtype, rc)
    for dtype in (-1, 6):
        rc, h = _create(lib, dtype, np.float32, 16, 4)
        assert rc == E_INVALID_ARGUMENT and not h.value
    rc, h = _create(lib, sd.RC32, np.float32, 0, 4)  # zero taps
    assert rc == E_INVALID_ARGUMENT and not h.value
    rc, h = _create(lib, sd.CC64, np.complex128, 16, 0)  # M = 0
    assert rc == E_INVALID_ARGUMENT and not h.value
    assert lib.sdsp_last_error()  # a message names the rule
    assert lib.sdsp_ddc_create(None, sd.RC32, None, 0, None, 1, 0) == E_INVALID_ARGUMENT


def test_no_device_fails_loudly():
    import solid_dsp_amd as sd
    lib = sd.lib()
    if sd.device_count() > 0:
        rc, h = _create(lib, sd.RC32, np.float32, 16, 4, device=sd.device_count() + 7)
    else:
        rc, h = _create(lib, sd.RC32, np.float32, 16, 4)
        with pytest.raises(sd.SdspError) as e:
            sd.DDC(np.ones(16, dtype=np.float32), 1.0, 4)
        assert e.value.code == E_NO_DEVICE
    assert rc == E_NO_DEVICE and not h.value  # no CPU fallback


def test_null_handle_calls():
    import solid_dsp_amd as sd
    lib = sd.lib()
    assert lib.sdsp_ddc_output_count(None, 1000) == 0
    assert lib.sdsp_ddc_state_len(None) == 0
    assert lib.sdsp_ddc_get_algo(None) == -1
    for call in (lambda: lib.sdsp_ddc_set_algo(None, 1), lambda: lib.sdsp_ddc_set_direction(None, 0),
                 lambda: lib.sdsp_ddc_set_frequency(None, 0.1), lambda: lib.sdsp_ddc_reset(None),
                 lambda: lib.sdsp_ddc_set_nco_state(None, 1, 2), lambda: lib.sdsp_ddc_synchronize(None),
                 lambda: lib.sdsp_ddc_execute_block_device(None, None, 0, None, None, None)):
        assert call() == E_INVALID_ARGUMENT
    lib.sdsp_ddc_destroy(None)  # a no-op
