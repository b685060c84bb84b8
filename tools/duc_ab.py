"""In-process A/B of the fused up-converter against the two handles it replaces (MI355X).

Three contestants on the c32 stream, ALGO_FMA, per shape (taps, M, L); real f32 taps (RC32) at the
two shapes the comparison is about, complex taps (CC32) at K = 16 for the record:
  a  fused     sd.DUC                                             reads 8/M B, writes 8 B per output
  b  pair      InterpolatingFIRFilter, then NCO.mix_block_device  24 + 8/M B per output
  c  interp    the InterpolatingFIRFilter alone on the same input the floor: a's bytes, no oscillator
Untimed settle passes over every contestant come before each round; within a round the order is
shuffled; each call is timed with device events on one stream (one call per window: a ratio
inside the recorded min .. max spread of its two medians is reported as indistinguishable, not as
a difference).  The fused output is compared with the pair's at the timed size: bit for bit on the
device, and as rel-RMS over the first 2^22 outputs on the host (0 is expected: same sums, same
product).  One JSON document on stdout and in --out.

    python tools/duc_ab.py --log2n 28 --rounds 12 --out profiles/r13/duc_ab.json
"""
import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("RC32", 32, 256), ("RC32", 8, 128), ("CC32", 8, 128)]  # cfg10's shape, a low-interpolation one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28, help="log2 of the outputs per call")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--settle", type=int, default=2, help="untimed passes over every contestant before each round")
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import solid_dsp_amd as sd
    from solid_dsp_amd.filter import firdes
    assert torch.cuda.is_available(), "duc_ab needs an MI355X"
    nout = 1 << args.log2n
    s = torch.cuda.current_stream()
    d_in = torch.empty(nout // 8, dtype=torch.complex64, device="cuda")
    sd.lib().sdsp_synth_f32_device(d_in.data_ptr(), 20250226, 0, 0, 2 * (nout // 8), None)
    # a writes out_a; b writes mid, then out_b; c writes mid as well (nobody reads it afterwards)
    out_a, out_b, mid = (torch.empty(nout, dtype=torch.complex64, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    rng = random.Random(args.seed)
    theta, dtheta = 0x9E3779B9, 0x0A3D70A3
    res = {"log2n_outputs": args.log2n, "rounds": args.rounds, "settle": args.settle, "algo": "FMA", "shapes": {}}
    for pair, M, L in SHAPES:
        n = nout // M
        h = firdes.firdes_kaiser(L, 0.5 / M, 80.0, 0.0).astype(np.float32)
        if pair == "CC32":
            h = (h * (1.0 + 0.25j)).astype(np.complex64)
        duc = sd.DUC(h, M, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
        nco = sd.NCO()
        itp_b = sd.InterpolatingFIRFilter(h, M, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
        itp_c = sd.InterpolatingFIRFilter(h, M, sample_dtype=np.complex64, algo=sd.ALGO_FMA)

        def run_a():
            duc.set_nco_state(theta, dtheta)
            duc.execute_block_device(d_in, n, out_a, s)

        def run_b():
            nco.set_state(theta, dtheta)
            itp_b.execute_block_device(d_in, n, mid, s)
            nco.mix_block_device(mid, nout, out_b, down=False, precision=0, stream=s)

        def run_c():
            itp_c.execute_block_device(d_in, n, mid, s)

        runs = {"a": run_a, "b": run_b, "c": run_c}
        # same results first: fresh windows, one call each
        run_a()
        run_b()
        torch.cuda.synchronize()
        same = bool(torch.equal(torch.view_as_real(out_a).view(torch.int32), torch.view_as_real(out_b).view(torch.int32)))
        k = min(nout, 1 << 22)
        ya, yb = out_a[:k].cpu().numpy().astype(np.complex128), out_b[:k].cpu().numpy().astype(np.complex128)
        rel = float(np.linalg.norm(ya - yb) / np.linalg.norm(yb))
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for _ in range(args.settle):
                for f in runs.values():
                    f()
            torch.cuda.synchronize()
            order = list(runs)
            rng.shuffle(order)
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                runs[k]()
                e1.record(s)
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in times.items()}
        byts = {"a": 8 * nout + 8 * n, "b": 24 * nout + 8 * n, "c": 8 * nout + 8 * n}
        lo = {k: float(np.min(v)) for k, v in times.items()}
        hi = {k: float(np.max(v)) for k, v in times.items()}

        def apart(p, q):  # the two spreads do not overlap
            return hi[p] < lo[q] or hi[q] < lo[p]

        res["shapes"][f"{pair}_M{M}_L{L}"] = {
            "fused_vs_pair_bit_identical": same,
            "fused_vs_pair_rel_rms": rel,
            "median_ms": med,
            "min_ms": lo,
            "max_ms": hi,
            "GBps": {k: byts[k] / (med[k] * 1e-3) / 1e9 for k in med},
            "a_over_b": med["a"] / med["b"],
            "a_over_b_by_bytes": byts["a"] / byts["b"],
            "a_over_c": med["a"] / med["c"],
            "a_b_distinguishable": apart("a", "b"),
            "a_c_distinguishable": apart("a", "c"),
        }
        del duc, nco, itp_b, itp_c
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
