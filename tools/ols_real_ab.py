"""Interleaved in-process A/B of the FIR paths of a real f32 handle (FIRFilter<f32, f32>) on a
long device-resident stream: the reference-order direct kernel (ALGO_EXACT), the fused
multiply-add direct kernel (ALGO_FMA) and overlap-save on packed segment pairs (ALGO_FFT,
kern_fir_ols_real.hip) in both lane shapes (SDSP_TUNE_OLS_KERNEL 0: 4-byte lanes, 3: 8-byte
lanes).  Shuffled order every round, median of rounds, untimed settle work first (guide §5.4
rule 24, as tools/ols_ab.py).

  python tools/ols_real_ab.py                       # 2^30 samples, 12 rounds
  python tools/ols_real_ab.py --rounds 20 --json profiles/r07/ols_real_ab.json

Workload: firdes_kaiser(256, 0.1, 80) taps as f32, scale 0.2, 2^30 f32 samples from
sdsp_synth_f32_device.  Per variant: ms, GS/s, GB/s at 8 B/sample (4 read + 4 written), the
fraction of 8 TB/s, and the rel-RMS against the f64 restatement over 4 random 4096-sample
windows recomputed on the host from the preceding inputs (as bench.py's parity).
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

TUNE_OLS_KERNEL = 14
HBM_BPS = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--settle", type=int, default=3, help="untimed passes over every variant before the rounds")
    ap.add_argument("--taps", type=int, default=256)
    ap.add_argument("--json", default=None, help="also write the result here")
    args = ap.parse_args()
    assert args.rounds >= 1

    import torch
    import oracle_lib as O
    import solid_dsp_amd as sd
    from solid_dsp_amd import FIRFilter
    from solid_dsp_amd.filter import firdes

    n, L = 1 << args.log2n, args.taps
    h = firdes.firdes_kaiser(L, 0.1, 80.0, 0.0).astype(np.float32)
    d_in = torch.empty(n, dtype=torch.float32, device="cuda")
    sd.lib().sdsp_synth_f32_device(d_in.data_ptr(), 20250226, 0, 0, n, None)
    torch.cuda.synchronize()

    def make(algo, kern=None):
        f = FIRFilter(h, np.float32(0.2), sample_dtype=np.float32, algo=algo, host_step=False)
        if kern is not None:
            f.set_tuning(TUNE_OLS_KERNEL, kern)
        return f

    variants = {"exact": make(sd.ALGO_EXACT), "fma": make(sd.ALGO_FMA),
                "fft_lanes4": make(sd.ALGO_FFT, 0), "fft_lanes8": make(sd.ALGO_FFT, 3)}
    s = torch.cuda.current_stream()
    d_out = torch.empty_like(d_in)

    # parity: 4 random output windows of every variant against the f64 restatement
    rng = np.random.default_rng(7)
    starts = [int(rng.integers(L, n - 4096)) for _ in range(4)]
    refs = []
    for st in starts:
        xs = d_in[st - (L - 1): st + 4096].cpu().numpy()
        refs.append(O.fir(O.RR64, h.astype(np.float64), 0.2).execute_block(xs.astype(np.float64))[L - 1:])
    rel = {}
    for k, f in variants.items():
        f.execute_block_device(d_in, n, d_out, s)
        torch.cuda.synchronize()
        worst = 0.0
        for st, ref in zip(starts, refs):
            ys = d_out[st: st + 4096].cpu().numpy().astype(np.float64)
            worst = max(worst, float(np.linalg.norm(ys - ref) / np.linalg.norm(ref)))
        rel[k] = worst
        f.reset()

    order = list(variants.items())
    for _ in range(args.settle):
        for k, f in order:
            f.execute_block_device(d_in, n, d_out, s)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        rng.shuffle(order)
        for k, f in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            f.execute_block_device(d_in, n, d_out, s)
            e1.record(s)
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))

    res = {"log2n": args.log2n, "taps": L, "rounds": args.rounds, "settle": args.settle, "variants": {}}
    for k, v in times.items():
        ms = float(np.median(v))
        bps = 8.0 * n / (ms * 1e-3)
        res["variants"][k] = {"median_ms": ms, "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                              "GSps": n / (ms * 1e-3) / 1e9, "GBps": bps / 1e9, "hbm_fraction": bps / HBM_BPS,
                              "rel_rms_vs_f64": rel[k]}
    direct = min(res["variants"]["exact"]["median_ms"], res["variants"]["fma"]["median_ms"])
    res["fft_over_best_direct"] = {k: direct / res["variants"][k]["median_ms"] for k in ("fft_lanes4", "fft_lanes8")}
    for k, r in res["variants"].items():
        print(f"{k:11s} {r['median_ms']:9.3f} ms  {r['GSps']:7.2f} GS/s  {r['GBps']:8.1f} GB/s  "
              f"{r['hbm_fraction']:.3f} of 8 TB/s  rel-RMS {r['rel_rms_vs_f64']:.3e}")
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
