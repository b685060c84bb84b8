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

from . import _handle as H
from . import _lib as L


class DDC(H.Oscillator, H.FirHandle):
    _family = "ddc"

    def __init__(self, taps, scale=1.0, decimation=1, sample_dtype=None, coef_dtype=None, device=0, channels=1,
                 algo=None):
        c = self._coefs(taps, sample_dtype, coef_dtype)
        s = np.array([scale], dtype=self.coef_dtype)
        h = C.c_void_p()
        L.check(L.lib().sdsp_ddc_create(C.byref(h), self.dtype, L.ptr(c), len(c), L.ptr(s), int(decimation),
                                        int(device)))
        self._adopt(h, device, channels, algo)  # algo None: the process default, ALGO_EXACT unless changed

    @classmethod
    def new(cls, taps, scale, decimation, **kw):
        return cls(taps, scale, decimation, **kw)

    # ---- configuration -------------------------------------------------
    set_channels, set_algo, get_algo = H.set_channels, H.set_algo, H.get_algo
    set_tuning = H.set_tuning  # SDSP_TUNE_DECIM_SEG, the polyphase kernel's group length

    def set_direction(self, up: bool):
        """False (default): mix_down; True: mix_up."""
        self._call("set_direction", 1 if up else 0)

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
        x, n = self._block_in(samples)
        y = self._block_out(self.output_count(n))
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
