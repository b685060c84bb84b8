"""MI355X: every kernel path of the receive chain (kern_rx.hip), case by case.

The tables and the launch rules they are built on are in tests/rx_cases.py; tests/test_rx_cases.py
shows (without a GPU) that they reach every path.  AutoCorrelator and the c64 NCO are bit-identical
to the CPU restatement (oracle/sdsp_oracle_rx.cpp), the c32 NCO to the unfused f32 model of
rx_cases.nco_model, the AGC bank within test_gpu_rx.AGC_RTOL of the restatement with squelch modes
and timers equal.
"""
import numpy as np
import pytest

import oracle_lib as O
import rx_cases as R
from gpu_util import to_dev, to_host
from test_gpu_rx import AGC_RTOL, _close

pytestmark = pytest.mark.gpu

C64, C128 = R.C64, R.C128
DT_IDS = {C64: "c64", C128: "c128"}


def _stream():
    import torch
    return torch.cuda.current_stream()


# ---------------------------------------------------------------- AutoCorrelator
def _acorr_handle(case, dt):
    import solid_dsp_amd as sd
    from solid_dsp_amd import _lib as L
    W, d, calls, knob, slots, ch = case
    g = sd.AutoCorrelator(W, d, dtype=dt, channels=ch)
    if knob:
        g.set_tuning(L.TUNE_ACORR_KERNEL, knob)
    if slots:
        g.set_tuning(L.TUNE_ACORR_SLOTS, slots)
    return g


def _acorr_case(case, dt):
    """the case's calls in order on one handle, every channel bit-identical to O.AutoCorr"""
    import torch
    W, d, calls, knob, slots, ch = case
    x = R.acorr_input(case, dt)
    g = _acorr_handle(case, dt)
    refs = [O.AutoCorr(W, d, dt) for _ in range(ch)]
    lo = 0
    for n in calls:
        blk = np.ascontiguousarray(x[:, lo:lo + n])
        d_in = to_dev(blk)
        d_out = torch.empty_like(d_in)
        g.execute_block_device(d_in, n, d_out, _stream())
        y = to_host(d_out)
        for c in range(ch):
            r = refs[c].execute_block(blk[c])
            assert y[c].tobytes() == r.tobytes(), (R.acorr_id(case), lo, n, c, int(np.argmax(y[c] != r)))
        lo += n
    return g, refs


def _params(cases):
    return [pytest.param(c, dt, id=f"{R.acorr_id(c)}-{DT_IDS[dt]}") for c in cases for dt in R.DTYPES]


@pytest.mark.parametrize("case,dt", _params(R.ACORR_BRANCH))
def test_acorr_pipelined_sum_branches(case, dt):
    """d = 3, every code shape of acorr_pipe_kernel's sum: a call with a leading edge tile on the
    history, three interior tiles and a ragged trailing tile, then a call of whole tiles"""
    first, second = R.case_plans(case)
    assert first["pipe"] and second["pipe"] and second["pipe"]["trailing"] == 0
    _acorr_case(case, dt)


@pytest.mark.parametrize("case,dt", _params(R.ACORR_DELAY))
def test_acorr_delay_boundaries(case, dt):
    """K = 16 at every delay limit (129 leaves the pipelined kernel, 257 leaves STAGE), and
    K = d = 128, the pipelined kernel's largest LDS and register footprint"""
    d = case[1]
    p = R.case_plans(case)[0]
    assert (p["pipe"] is not None) == (d <= R.K_PIPE_D) and p["stage"] == (d <= R.K_DMAX)
    _acorr_case(case, dt)


@pytest.mark.parametrize("case,dt", _params(R.ACORR_NO_INTERIOR))
def test_acorr_no_interior_tile(case, dt):
    """pipeline-eligible, t_hi == t_lo: the whole call on the one-shot kernel"""
    (p,) = R.case_plans(case)
    assert p["pipe_eligible"] and p["pipe"] is None and p["t_hi"] == p["t_lo"]
    _acorr_case(case, dt)


@pytest.mark.parametrize("case,dt", _params(R.ACORR_ONESHOT))
def test_acorr_oneshot_chunks(case, dt):
    """K > 128 on the default knob: one, two and three chunks, later chunks on either side of
    cj >= 8, the staged (d <= 256) and the two-load (d = 300) form"""
    assert all(p["pipe"] is None for p in R.case_plans(case))
    _acorr_case(case, dt)


@pytest.mark.parametrize("case,dt", _params(R.ACORR_KNOB))
def test_acorr_kernel_knobs(case, dt):
    """SDSP_TUNE_ACORR_KERNEL 1 and 2: the one-shot kernel where the default runs the pipelined one"""
    _acorr_case(case, dt)


@pytest.mark.parametrize("case,dt", _params(R.ACORR_SLOTS))
def test_acorr_many_tiles_per_wave(case, dt):
    """SDSP_TUNE_ACORR_SLOTS = 1: eight waves per channel, so each walks up to four tiles (the
    rotated stage(), the look-ahead load past its eighth's end) and the eighths hold unequal tile
    counts, two of them none at the shorter length; two channels"""
    (p,) = R.case_plans(case)
    assert p["pipe"]["G"] == 8 and len(set(p["pipe"]["eighths"])) > 1
    _acorr_case(case, dt)


@pytest.mark.parametrize("slots", [3, 9, 16, 65536])
def test_acorr_slots_knob_other_values(slots):
    """slots that are no multiple of eight (rounded up: the kernel divides its grid by 8), more
    than one wave per eighth, and more slots than tiles (the automatic launch)"""
    case = (64, 16, (R.N_SLOTS[0],), 0, slots, 2)
    G = R.case_plans(case)[0]["pipe"]["G"]
    assert G == {3: 8, 9: 16, 16: 16, 65536: 32}[slots]
    _acorr_case(case, C64)


def test_acorr_tuning_rejects_other_values():
    import solid_dsp_amd as sd
    from solid_dsp_amd import _lib as L
    assert (L.TUNE_ACORR_KERNEL, L.TUNE_ACORR_SLOTS) == (R.TUNE_ACORR_KERNEL, R.TUNE_ACORR_SLOTS)
    g = sd.AutoCorrelator(64, 16, dtype=C64)
    for v in (1, 8, 65536, 0):
        g.set_tuning(L.TUNE_ACORR_SLOTS, v)
    for key, v in ((L.TUNE_ACORR_SLOTS, -1), (L.TUNE_ACORR_SLOTS, 65537), (L.TUNE_ACORR_SLOTS, 1 << 30),
                   (L.TUNE_ACORR_KERNEL, 3), (L.TUNE_ACORR_KERNEL, -1), (L.TUNE_AGC_KERNEL, 0), (31, 0)):
        with pytest.raises(sd.SdspError):
            g.set_tuning(key, v)


@pytest.mark.parametrize("case,dt", _params(R.ACORR_CHANNELS))
def test_acorr_channels_short_blocks_and_write_device(case, dt):
    """three channels on device buffers, calls shorter than the window first (history and input
    mix in ext_at and in the energy sum): execute() and get_energy() per channel after every call,
    and write_device of the same data on a second handle leaves the same state"""
    import torch
    W, d, calls, knob, slots, ch = case
    x = R.acorr_input(case, dt)
    g, w = _acorr_handle(case, dt), _acorr_handle(case, dt)
    refs = [O.AutoCorr(W, d, dt) for _ in range(ch)]
    lo = 0
    for n in calls:
        blk = np.ascontiguousarray(x[:, lo:lo + n])
        d_in = to_dev(blk)
        d_out = torch.empty_like(d_in)
        g.execute_block_device(d_in, n, d_out, _stream())
        w.write_device(d_in, n, _stream())
        y = to_host(d_out)
        cur, e = g.execute(), g.get_energy()
        for c in range(ch):
            assert y[c].tobytes() == refs[c].execute_block(blk[c]).tobytes(), (lo, n, c)
            assert cur[c].tobytes() == refs[c].execute().tobytes(), (lo, n, c)
            er = refs[c].get_energy()
            assert abs(e[c] - er) <= 1e-12 * max(er, 1e-300) + 1e-300, (lo, n, c, e[c], er)
        assert w.execute().tobytes() == cur.tobytes(), (lo, n)
        assert w.get_energy().tobytes() == e.tobytes(), (lo, n)
        lo += n


# ---------------------------------------------------------------- NCO
def _sentinel(count, dt):
    """`count` samples of a bit pattern with all 32-bit words distinct (quiet NaNs as f32)"""
    words = count * (2 if dt == C64 else 4)
    w = (np.arange(words, dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(0x7FC00000)
    return w.view(np.float32).view(dt) if dt == C64 else w.view(np.uint64).view(np.float64).view(dt)


def _nco_call(g, x, n, off_in, off_out, down, prec, want, tag):
    """one mix_block_device of x[:n] through pointers `off` samples past 16-byte alignment; the n
    outputs equal `want` bit for bit and every byte of the buffer around them is unchanged"""
    dt = C64 if prec == 0 else C128
    guard = R.NCO_GUARD
    src = np.zeros(n + 2, dtype=dt)
    src[off_in:off_in + n] = x[:n]
    buf = _sentinel(2 * guard + n + 2, dt).copy()
    d_src, d_buf = to_dev(src), to_dev(buf)
    lo = guard + off_out
    assert d_src.data_ptr() % 16 == 0 and d_buf.data_ptr() % 16 == 0
    th0, dth = g.state()
    g.mix_block_device(d_src[off_in:], n, d_buf[lo:], down=down, precision=prec, stream=_stream())
    got = to_host(d_buf)
    out = got[lo:lo + n]
    assert out.dtype == want.dtype and len(want) == n
    differ = np.flatnonzero(out.view(np.uint32) != want.view(np.uint32))
    assert out.tobytes() == want.tobytes(), (tag, "words that differ", len(differ), "first sample",
                                             int(differ[0]) // (2 if prec == 0 else 4))
    assert got[:lo].tobytes() == buf[:lo].tobytes(), (tag, "bytes before the output changed")
    assert got[lo + n:].tobytes() == buf[lo + n:].tobytes(), (tag, "bytes after the output changed")
    assert g.state() == (R.nco_end_state(th0, dth, n), dth), tag


@pytest.mark.parametrize("down", [False, True], ids=["up", "down"])
@pytest.mark.parametrize("off_in,off_out", R.NCO_SHAPES, ids=["v2", "in-off", "out-off", "both-off"])
def test_nco_c32_bit_identical_to_f32_model(off_in, off_out, down):
    """the c32 kernel, both lane widths and every cause of the narrow one, lengths round a
    workgroup's 2048 vectors: bit-identical to the unfused f32 model, guard samples untouched"""
    import solid_dsp_amd as sd
    x = R.crand(71, max(R.NCO_N), C64)
    g = sd.NCO()
    th0, dth = 0x3C6EF372, 0x0B4E1A97
    for n in R.NCO_N:
        assert R.nco_plan(n, 0, off_in == 0, off_out == 0)["V"] == (2 if (off_in, off_out) == (0, 0) else 1)
        g.set_state(th0, dth)
        want = R.nco_model(x[:n], th0, dth, down, np.float32)
        _nco_call(g, x, n, off_in, off_out, down, 0, want, (n, off_in, off_out, down))


@pytest.mark.parametrize("down", [False, True], ids=["up", "down"])
def test_nco_c64_bit_identical_to_restatement(down):
    import solid_dsp_amd as sd
    x = R.crand(72, max(R.NCO_N), C128)
    g = sd.NCO()
    th0, dth = 0x3C6EF372, 0x0B4E1A97
    for n in R.NCO_N:
        for off in (0, 1):
            g.set_state(th0, dth)
            o = O.Nco()
            o.set_state(th0, dth)
            want = o.mix_block(x[:n], down)
            _nco_call(g, x, n, off, off, down, 1, want, (n, off, down))
            assert g.state() == o.state()


@pytest.mark.parametrize("down", [False, True], ids=["up", "down"])
@pytest.mark.parametrize("th0,dth", R.NCO_PHASES, ids=["wraps", "rounds-up", "crosses"])
def test_nco_phase_wrap_on_device(th0, dth, down):
    """theta near 2^32 with a large step, the table index rounding up through zero, and the
    rounding point crossed inside the call; the state after the call is theta0 + n dtheta mod 2^32"""
    import solid_dsp_amd as sd
    n = 4099
    g = sd.NCO()
    x32, x64 = R.crand(73, n, C64), R.crand(74, n, C128)
    o = O.Nco()
    o.set_state(th0, dth)
    g.set_state(th0, dth)
    _nco_call(g, x64, n, 0, 0, down, 1, o.mix_block(x64, down), ("c64", hex(th0)))
    assert g.state() == o.state() == (R.nco_end_state(th0, dth, n), dth)
    for off_in, off_out in ((0, 0), (1, 1)):
        g.set_state(th0, dth)
        want = R.nco_model(x32, th0, dth, down, np.float32)
        _nco_call(g, x32, n, off_in, off_out, down, 0, want, ("c32", hex(th0), off_in))


# ---------------------------------------------------------------- AGC
def _agc_call(g, refs, blk, cplx, tag):
    """one call of a bank on device buffers; every channel against its restatement"""
    import torch
    n = blk.shape[1]
    d_in = to_dev(blk)
    d_out = torch.empty_like(d_in)
    g.execute_block_device(d_in, n, d_out, complex_=cplx, stream=_stream())
    y = to_host(d_out)
    for c, o in enumerate(refs):
        r = o.execute_block(blk[c])
        assert _close(y[c], r), (tag, c, float(np.max(np.abs(y[c] - r))), float(np.max(np.abs(r))))
        st = g.state(c)
        assert abs(st.gain - o.get_gain()) <= AGC_RTOL * o.get_gain(), (tag, c, st.gain, o.get_gain())
        assert st.squelch_mode == o.get_mode(), (tag, c, st.squelch_mode, o.get_mode())
        assert st.squelch_timer == o.get_timer(), (tag, c)
    return y


def _agc_edge_pair(channels, knob):
    import solid_dsp_amd as sd
    from solid_dsp_amd import _lib as L
    g = sd.AGC(channels=channels)
    g.set_tuning(L.TUNE_AGC_KERNEL, knob)
    g.squelch_enable()
    g.squelch_set_threshold(-30.0)
    g.squelch_set_timeout(5)
    g.set_bandwidth(0.05)
    refs = []
    for _ in range(channels):
        o = O.Agc()
        o.squelch(1)
        o.squelch_set_threshold(-30.0)
        o.squelch_set_timeout(5)
        assert o.set_bandwidth(0.05) == 0
        refs.append(o)
    return g, refs


def _agc_edge_stream(channels, knob, cplx):
    x = R.agc_edge_input(channels, cplx)
    g, refs = _agc_edge_pair(channels, knob)
    lo = 0
    for n in R.AGC_EDGE_CALLS:
        _agc_call(g, refs, np.ascontiguousarray(x[:, lo:lo + n]), cplx, (lo, n))
        lo += n


@pytest.mark.parametrize("knob", [0, 1], ids=["pipe", "plain"])
@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "real"])
def test_agc_chunk_edges_bank(cplx, knob):
    """65 channels (a full workgroup and one of a single lane), real and complex samples on both
    kernels: one stream in calls round the chunk sizes (no whole chunk, whole chunks exactly, a
    ragged chunk after whole ones), every channel compared after every call"""
    _agc_edge_stream(R.AGC_EDGE_CHANNELS, knob, cplx)


@pytest.mark.parametrize("channels", R.AGC_EDGE_EXTRA_CHANNELS)
def test_agc_chunk_edges_channel_counts(channels):
    """the pipelined complex form with 1, 63, 64 and 130 channels: the descriptors' row bound"""
    _agc_edge_stream(channels, 0, True)


def _agc_het_bank(knob):
    import solid_dsp_amd as sd
    from solid_dsp_amd import _lib as L
    ps = R.agc_het_params()
    g = sd.AGC(channels=len(ps))
    g.set_tuning(L.TUNE_AGC_KERNEL, knob)
    for c, p in enumerate(ps):
        st = g.state(c)
        st.bandwidth = st.alpha = p["bandwidth"]
        st.scale = p["scale"]
        st.squelch_mode = R.SQ_ENABLED if p["squelch"] else R.SQ_DISABLED
        st.squelch_threshold = p["threshold"]
        st.squelch_timeout = p["timeout"]
        st.lock = 1 if p["lock"] else 0
        g.set_state(st, c)
    return g, [R.agc_oracle(O, p) for p in ps]


@pytest.mark.parametrize("knob", [0, 1], ids=["pipe", "plain"])
@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "real"])
def test_agc_heterogeneous_bank(cplx, knob):
    """70 channels, each with its own bandwidth, scale, squelch switch, threshold and timeout,
    every seventh locked: lanes of one wave in different squelch modes, at the gain clamp and in
    the energy freeze at once (tests/test_rx_cases.py shows the inputs get there)"""
    x = R.agc_het_input(cplx)
    g, refs = _agc_het_bank(knob)
    lo = 0
    for n in R.AGC_HET_CALLS:
        _agc_call(g, refs, np.ascontiguousarray(x[:, lo:lo + n]), cplx, (lo, n))
        lo += n
    scales = g.get_scale()
    assert [float(s) for s in scales] == [p["scale"] for p in R.agc_het_params()]


@pytest.mark.parametrize("n", R.AGC_INIT_N)
@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "real"])
def test_agc_init_bank(cplx, n):
    """init on a 70-channel bank: levels and gains bit-identical to the restatement (an in-order
    f64 sum, one divide, one square root: correctly rounded on both sides), then a block"""
    import solid_dsp_amd as sd
    ch = R.AGC_HET_CHANNELS
    x = R.agc_init_input(n, cplx)
    g = sd.AGC(channels=ch)
    refs = [O.Agc() for _ in range(ch)]
    lv = g.init(x)
    gains = g.get_gain()
    for c, o in enumerate(refs):
        rc, l = o.init(x[c])
        assert rc == 0
        assert np.float64(lv[c]).tobytes() == np.float64(l).tobytes(), (c, lv[c], l)
        assert np.float64(gains[c]).tobytes() == np.float64(o.get_gain()).tobytes(), (c, gains[c], o.get_gain())
        assert g.state(c).energy_estimate == 1.0
    _agc_call(g, refs, R.agc_init_input(40, cplx), cplx, "block after init")


@pytest.mark.parametrize("knob", [0, 1], ids=["pipe", "plain"])
@pytest.mark.parametrize("cplx", [True, False], ids=["complex", "real"])
def test_agc_nan_sample(cplx, knob):
    """one NaN into the middle channel of three, mid-stream: its output is NaN where the
    restatement's is and within the bound elsewhere (the energy estimate stays NaN, so the gain
    freezes and later outputs are finite again), modes and timers equal, neighbours untouched"""
    import torch
    n, cuts, at = 100, (0, 37, 100), 50
    rng = np.random.default_rng(81)
    x = 0.05 * rng.standard_normal((3, n))
    if cplx:
        x = x + 0.05j * rng.standard_normal((3, n))
    xn = x.copy()
    xn[1, at] = complex(np.nan, x[1, at].imag) if cplx else np.nan
    g, refs = _agc_edge_pair(3, knob)
    clean, _ = _agc_edge_pair(3, knob)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        blk, cblk = np.ascontiguousarray(xn[:, lo:hi]), np.ascontiguousarray(x[:, lo:hi])
        d_in, d_cin = to_dev(blk), to_dev(cblk)
        d_out, d_cout = torch.empty_like(d_in), torch.empty_like(d_cin)
        g.execute_block_device(d_in, hi - lo, d_out, complex_=cplx, stream=_stream())
        clean.execute_block_device(d_cin, hi - lo, d_cout, complex_=cplx, stream=_stream())
        y, yc = to_host(d_out), to_host(d_cout)
        for c, o in enumerate(refs):
            r = o.execute_block(blk[c])
            yv, rv = y[c].view(np.float64), r.view(np.float64)
            assert np.array_equal(np.isnan(yv), np.isnan(rv)), (lo, c)
            bad = np.isnan(r)
            assert int(bad.sum()) == (1 if c == 1 and lo <= at < hi else 0), (lo, c)
            assert _close(np.where(bad, 0, y[c]), np.where(bad, 0, r)), (lo, c)
            st = g.state(c)
            assert abs(st.gain - o.get_gain()) <= AGC_RTOL * o.get_gain(), (lo, c)
            assert np.isnan(st.energy_estimate) == np.isnan(o.get_energy()), (lo, c)
            assert np.isnan(st.energy_estimate) == (c == 1 and hi > at), (lo, c)
            assert st.squelch_mode == o.get_mode() and st.squelch_timer == o.get_timer(), (lo, c)
        for c in (0, 2):  # the neighbours: the same bits as a bank that never saw the NaN
            assert y[c].tobytes() == yc[c].tobytes(), (lo, c)
