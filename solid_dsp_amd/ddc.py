"""Digital down-converter on MI355X: ``NCO`` mix-down fused into ``DecimatingFIRFilter``.

A build-defined composition of two reference objects (src/nco/mod.rs,
src/filter/fir/decim.rs), as the channeliser is: ``DDC(taps, scale, M)`` with an
oscillator ``(theta, delta_theta)`` computes, sample for sample,

    v = nco.mix_down(x[i]); nco.step(); decimator.execute(v)

in one pass over the input (``kern_ddc.hip``): the mixed stream is never written
to memory.  ``ALGO_EXACT`` (the default) is bit-identical to
``NCO.mix_block_device(down=True)`` followed by an ``ALGO_EXACT``
``DecimatingFIRFilter``; ``ALGO_FMA`` runs the polyphase kernel.  Samples are
complex (complex64 / complex128); taps real or complex of the same precision.
A block object: there is no per-sample ``push``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .filter.fir import _coef_array, _default_sample


class DDC:
    def __init__(self, taps, scale=1.0, decimation=1, sample_dtype=None, coef_dtype=None, device=0, channels=1,
                 algo=None):
        c = _coef_array(taps, coef_dtype)
        if sample_dtype is None:
            sample_dtype = _default_sample(c.dtype)
        self.dtype = L.dtype_code(c.dtype, sample_dtype)
        self.coef_dtype = L.COEF_DTYPE[self.dtype]
        self.sample_dtype = L.SAMPLE_DTYPE[self.dtype]
        s = np.array([scale], dtype=self.coef_dtype)
        h = C.c_void_p()
        L.check(L.lib().sdsp_ddc_create(C.byref(h), self.dtype, L.ptr(c), len(c), L.ptr(s), int(decimation),
                                        int(device)))
        self._h = h
        self.device = device
        self.channels = 1
        if channels != 1:
            self.set_channels(channels)
        if algo is not None:  # default: the process default, ALGO_EXACT unless changed
            self.set_algo(algo)

    @classmethod
    def new(cls, taps, scale, decimation, **kw):
        return cls(taps, scale, decimation, **kw)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            L.lib().sdsp_ddc_destroy(h)
            self._h = None

    # ---- configuration -------------------------------------------------
    def set_channels(self, channels: int):
        L.check(L.lib().sdsp_ddc_set_channels(self._h, channels))
        self.channels = channels

    def set_algo(self, algo: int):
        L.check(L.lib().sdsp_ddc_set_algo(self._h, int(algo)))

    def get_algo(self) -> int:
        return int(L.lib().sdsp_ddc_get_algo(self._h))

    def set_direction(self, up: bool):
        """False (default): mix_down; True: mix_up."""
        L.check(L.lib().sdsp_ddc_set_direction(self._h, 1 if up else 0))

    def set_tuning(self, key: int, value: int):
        """SDSP_TUNE_DECIM_SEG, the polyphase kernel's group length (performance only)"""
        L.check(L.lib().sdsp_ddc_set_tuning(self._h, int(key), int(value)))

    def clone(self):
        h = C.c_void_p()
        L.check(L.lib().sdsp_ddc_clone(self._h, C.byref(h)))
        obj = type(self).__new__(type(self))
        obj.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_h"})
        obj._h = h
        return obj

    __copy__ = clone

    def reset(self):
        L.check(L.lib().sdsp_ddc_reset(self._h))

    # ---- oscillator (NCO setters, src/nco/mod.rs:59-86) -----------------
    def set_frequency(self, delta_theta: float):
        L.check(L.lib().sdsp_ddc_set_frequency(self._h, float(delta_theta)))

    def adjust_frequency(self, dt: float):
        L.check(L.lib().sdsp_ddc_adjust_frequency(self._h, float(dt)))

    def set_phase(self, phi: float):
        L.check(L.lib().sdsp_ddc_set_phase(self._h, float(phi)))

    def adjust_phase(self, delta_phi: float):
        L.check(L.lib().sdsp_ddc_adjust_phase(self._h, float(delta_phi)))

    def nco_state(self):
        """(theta, delta_theta), the raw u32 registers"""
        th, dt = C.c_uint32(), C.c_uint32()
        L.check(L.lib().sdsp_ddc_get_nco_state(self._h, C.byref(th), C.byref(dt)))
        return th.value, dt.value

    def set_nco_state(self, theta: int, delta_theta: int):
        L.check(L.lib().sdsp_ddc_set_nco_state(self._h, int(theta) & 0xFFFFFFFF, int(delta_theta) & 0xFFFFFFFF))

    # ---- delay line -----------------------------------------------------
    def get_state(self):
        """(delay line [channels * (len - 1)] of mixed samples, decimator phase)"""
        n = int(L.lib().sdsp_ddc_state_len(self._h))
        hist = np.zeros(n, dtype=self.sample_dtype)
        phase = C.c_size_t(0)
        L.check(L.lib().sdsp_ddc_get_state(self._h, L.ptr(hist), C.byref(phase)))
        return hist, phase.value

    def set_state(self, hist, phase=0):
        hist = np.ascontiguousarray(hist, dtype=self.sample_dtype)
        L.check(L.lib().sdsp_ddc_set_state(self._h, L.ptr(hist), phase))

    # ---- blocks ----------------------------------------------------------
    def output_count(self, n: int) -> int:
        return int(L.lib().sdsp_ddc_output_count(self._h, n))

    def execute_block(self, samples) -> np.ndarray:
        """Host samples (channel-major [channels, n] when channels > 1) -> the decimated outputs."""
        x = np.ascontiguousarray(samples, dtype=self.sample_dtype)
        n = x.shape[-1] if x.ndim else 0
        if self.channels > 1 and (x.ndim != 2 or x.shape[0] != self.channels):
            raise ValueError("multi-channel input must be [channels, n]")
        nout = self.output_count(n)
        y = np.zeros((self.channels, nout), dtype=self.sample_dtype) if self.channels > 1 else \
            np.zeros(nout, dtype=self.sample_dtype)
        got = C.c_size_t(0)
        L.check(L.lib().sdsp_ddc_execute_block(self._h, L.ptr(x) if x.size else None, n,
                                               L.ptr(y) if y.size else None, C.byref(got)))
        return y

    def execute_block_device(self, d_in, n: int, d_out, stream=None) -> int:
        """Device-resident block: d_in / d_out are torch tensors or raw device pointers
        (channel-major, n samples per channel in, output_count(n) per channel out)."""
        got = C.c_size_t(0)
        pin = L.device_ptr(d_in, self.sample_dtype, self.channels * n, self.device, "input")
        pout = L.device_ptr(d_out, self.sample_dtype, self.channels * self.output_count(n), self.device, "output")
        L.check(L.lib().sdsp_ddc_execute_block_device(self._h, pin, n, pout, C.byref(got), L.stream_handle(stream)))
        return got.value

    def synchronize(self):
        L.check(L.lib().sdsp_ddc_synchronize(self._h))
