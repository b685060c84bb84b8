"""Interleaved in-process A/B of the FIR paths of a long-filter RC32 handle (f32 taps, complex f32
samples, more than 3841 taps) on a device-resident stream: the reference-order direct kernel
(ALGO_EXACT), the fused multiply-add direct kernel (ALGO_FMA) and the three-pass overlap-save
path (ALGO_FFT, kern_fir_ols_long.hip) at its automatic transform size and one size up and down
(SDSP_TUNE_OLS_LONG_LOG2N).  Shuffled order every round, median of rounds, untimed settle work
first (as tools/ols_real_ab.py).

  python tools/ols_long_ab.py                       # 2^26 samples, L in 3842 16385 65537 1048577
  python tools/ols_long_ab.py --rounds 9 --json profiles/r10/ols_long_ab.json

Workload: firdes_kaiser(L, 0.1, 80) taps as f32, scale 0.2, 2^26 complex samples from
sdsp_synth_f32_device.  The direct kernels cost L multiply-adds per output: they run on a prefix
of the stream of at most --direct-macs multiply-adds (a power of two of samples, at least 2 L),
and their rates are per sample of that prefix.  Per variant: samples, ms, GS/s, the bytes per
output the three passes imply ((5 N + V + N table reads) * 8 / V; 16 for the direct kernels) and
the rel-RMS over four random 4096-output windows (past the first L - 1 outputs) recomputed in
complex128 on the host from the preceding inputs.

A second table (--auto-lengths) times single calls of 2^16 .. 2^20 samples at the shortest long
filter (L = 3842) on the reference-order kernel and on the long path: the block length from which
SDSP_ALGO_AUTO should take the long path (runtime.cpp kOlsLongAutoMin).
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

TUNE_LOG2N = 22
WIN = 4096


def auto_log2n(L):
    lg = 14
    while (1 << lg) < 4 * (L - 1):
        lg += 1
    return lg


def window_ref(h, scale, xs):
    """the last WIN outputs of the filter over xs (len(h) - 1 + WIN inputs), complex128 FFT convolution"""
    L = len(h)
    M = 1 << int(len(xs) + L - 1).bit_length()
    g = h[::-1].astype(np.complex128) * scale
    return np.fft.ifft(np.fft.fft(xs.astype(np.complex128), M) * np.fft.fft(g, M))[L - 1:L - 1 + WIN]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--taps", type=int, nargs="+", default=[3842, 16385, 65537, 1048577])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--settle", type=int, default=1, help="untimed passes over every variant before the rounds")
    ap.add_argument("--direct-macs", type=int, default=1 << 41,
                    help="the direct kernels run on a prefix of at most this many multiply-adds")
    ap.add_argument("--auto-lengths", type=int, nargs="*", default=[16, 17, 18, 19, 20],
                    help="log2 block lengths of the AUTO threshold table (L = 3842); none to skip")
    ap.add_argument("--auto-calls", type=int, default=10, help="back-to-back calls per timed sample of that table")
    ap.add_argument("--json", default=None, help="also write the result here")
    args = ap.parse_args()
    assert args.rounds >= 1

    import torch
    import solid_dsp_amd as sd
    from solid_dsp_amd import FIRFilter
    from solid_dsp_amd.filter import firdes

    n = 1 << args.log2n
    d_in = torch.empty(n, dtype=torch.complex64, device="cuda")
    sd.lib().sdsp_synth_f32_device(d_in.data_ptr(), 20250226, 0, 0, 2 * n, None)
    torch.cuda.synchronize()
    d_out = torch.empty_like(d_in)
    s = torch.cuda.current_stream()
    rng = np.random.default_rng(7)

    def timed(f, count, calls=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(calls):
            f.execute_block_device(d_in, count, d_out, s)
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    res = {"log2n": args.log2n, "rounds": args.rounds, "settle": args.settle, "direct_macs": args.direct_macs,
           "filters": {}}
    for L in args.taps:
        h = firdes.firdes_kaiser(L, 0.1, 80.0, 0.0).astype(np.float32)

        def make(algo, lg=None):
            f = FIRFilter(h, np.float32(0.2), sample_dtype=np.complex64, algo=algo, host_step=False)
            if lg is not None:
                f.set_tuning(TUNE_LOG2N, lg)
            return f

        nd = n
        while nd > WIN and nd * L > args.direct_macs and nd >= 4 * L:  # (at least 2 L samples: the windows below)
            nd //= 2
        lg0 = auto_log2n(L)
        variants = {"exact": (make(sd.ALGO_EXACT), nd), "fma": (make(sd.ALGO_FMA), nd)}
        for lg in (lg0 - 1, lg0, lg0 + 1):
            if 13 <= lg <= 22 and (1 << lg) >= 2 * (L - 1):
                variants[f"long_2^{lg}" + ("_auto" if lg == lg0 else "")] = (make(sd.ALGO_FFT, lg), n)

        # parity: 4 random output windows inside every variant's block, past the first L - 1
        # outputs (while the delay line fills, the output is a partial sum far below the level
        # that the error of a segment is relative to)
        starts = [int(rng.integers(L - 1, nd - WIN)) for _ in range(4)]
        refs = []
        for st in starts:
            lo = st - (L - 1)
            xs = np.zeros(L - 1 + WIN, dtype=np.complex64)
            xs[max(0, -lo):] = d_in[max(lo, 0): st + WIN].cpu().numpy()
            refs.append(window_ref(h, 0.2, xs))
        rel = {}
        for k, (f, cnt) in variants.items():
            f.execute_block_device(d_in, cnt, d_out, s)
            torch.cuda.synchronize()
            worst = 0.0
            for st, ref in zip(starts, refs):
                ys = d_out[st: st + WIN].cpu().numpy().astype(np.complex128)
                worst = max(worst, float(np.linalg.norm(ys - ref) / np.linalg.norm(ref)))
            rel[k] = worst
            f.reset()

        order = list(variants.items())
        for _ in range(args.settle):
            for k, (f, cnt) in order:
                f.execute_block_device(d_in, cnt, d_out, s)
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            rng.shuffle(order)
            for k, (f, cnt) in order:
                times[k].append(timed(f, cnt))

        out = {}
        for k, (f, cnt) in variants.items():
            ms = float(np.median(times[k]))
            nfft, valid = f.ols_info()
            long_ = k.startswith("long")
            out[k] = {"samples": cnt, "median_ms": ms, "min_ms": float(np.min(times[k])),
                      "max_ms": float(np.max(times[k])), "GSps": cnt / (ms * 1e-3) / 1e9,
                      "nfft": nfft if long_ else 0, "valid": valid if long_ else 0,
                      "bytes_per_output": (5 * nfft + valid + nfft) * 8.0 / valid if long_ else 16.0,
                      "rel_rms_vs_f64": rel[k]}
            out[k]["GBps"] = out[k]["GSps"] * out[k]["bytes_per_output"]
        res["filters"][str(L)] = out
        print(f"L = {L}")
        for k, r in out.items():
            print(f"  {k:15s} {r['samples']:9d} samples {r['median_ms']:10.3f} ms  {r['GSps']:8.3f} GS/s  "
                  f"{r['bytes_per_output']:6.1f} B/output  {r['GBps']:8.1f} GB/s  rel-RMS {r['rel_rms_vs_f64']:.3e}")
        del variants, order

    if args.auto_lengths:
        L = 3842
        h = firdes.firdes_kaiser(L, 0.1, 80.0, 0.0).astype(np.float32)
        pair = {"exact": FIRFilter(h, np.float32(0.2), sample_dtype=np.complex64, algo=sd.ALGO_EXACT, host_step=False),
                "long": FIRFilter(h, np.float32(0.2), sample_dtype=np.complex64, algo=sd.ALGO_FFT, host_step=False)}
        table = {}
        for lg in args.auto_lengths:
            cnt = 1 << lg
            order = list(pair.items())
            for k, f in order:
                timed(f, cnt, args.auto_calls)
            t = {k: [] for k in pair}
            for _ in range(max(args.rounds, 9)):
                rng.shuffle(order)
                for k, f in order:
                    t[k].append(timed(f, cnt, args.auto_calls))
            table[str(cnt)] = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
            print(f"n = 2^{lg}: exact {table[str(cnt)]['exact']:9.1f} us/call   long {table[str(cnt)]['long']:9.1f} us/call")
        res["auto_threshold_us_per_call"] = table

    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
