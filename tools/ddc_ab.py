"""In-process A/B of the fused down-converter against the two handles it replaces (MI355X).

Three contestants on the c32 stream, ALGO_FMA, per shape (taps, M, L); real f32 taps (RC32) at the
two shapes the comparison is about, complex taps (CC32) at K = 16 for the record:
  a  fused     sd.DDC                                          reads 8 B, writes 8/M B per input
  b  pair      NCO.mix_block_device, then DecimatingFIRFilter  24 + 8/M B per input
  c  decim     the DecimatingFIRFilter alone on the same input the floor: a's bytes, no oscillator
Untimed settle passes over every contestant come before each round; within a round the order is
shuffled; each call is timed with device events on one stream (one call per window: a ratio
inside the recorded min .. max spread of its two medians is reported as indistinguishable, not as
a difference).  The fused output is compared with the pair's at the timed size (rel-RMS; it is 0
where both take the same lane shape: same product, same walk).  One JSON document on stdout and
in --out.

    python tools/ddc_ab.py --log2n 28 --rounds 12 --out profiles/r12/ddc_ab.json
"""
import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("RC32", 32, 256), ("RC32", 8, 128), ("CC32", 8, 128)]  # cfg4's shape, a low-decimation one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--settle", type=int, default=2, help="untimed passes over every contestant before each round")
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import solid_dsp_amd as sd
    from solid_dsp_amd.filter import firdes
    assert torch.cuda.is_available(), "ddc_ab needs an MI355X"
    n = 1 << args.log2n
    s = torch.cuda.current_stream()
    d_in = torch.empty(n, dtype=torch.complex64, device="cuda")
    sd.lib().sdsp_synth_f32_device(d_in.data_ptr(), 20250226, 0, 0, 2 * n, None)
    d_mix = torch.empty(n, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    rng = random.Random(args.seed)
    theta, dtheta = 0x9E3779B9, 0x0A3D70A3
    res = {"log2n": args.log2n, "rounds": args.rounds, "settle": args.settle, "algo": "FMA", "shapes": {}}
    for pair, M, L in SHAPES:
        h = firdes.firdes_kaiser(L, 0.5 / M, 80.0, 0.0).astype(np.float32)
        scale = np.float32(1.0)
        if pair == "CC32":
            h, scale = (h * (1.0 + 0.25j)).astype(np.complex64), np.complex64(1.0)
        ddc = sd.DDC(h, scale, M, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
        nco = sd.NCO()
        dec_b = sd.DecimatingFIRFilter(h, scale, M, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
        dec_c = sd.DecimatingFIRFilter(h, scale, M, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
        outs = {k: torch.empty(n // M, dtype=torch.complex64, device="cuda") for k in "abc"}

        def run_a():
            ddc.set_nco_state(theta, dtheta)
            ddc.execute_block_device(d_in, n, outs["a"], s)

        def run_b():
            nco.set_state(theta, dtheta)
            nco.mix_block_device(d_in, n, d_mix, down=True, precision=0, stream=s)
            dec_b.execute_block_device(d_mix, n, outs["b"], s)

        def run_c():
            dec_c.execute_block_device(d_in, n, outs["c"], s)

        runs = {"a": run_a, "b": run_b, "c": run_c}
        # same results first: fresh delay lines, one call each
        run_a()
        run_b()
        torch.cuda.synchronize()
        ya, yb = outs["a"].cpu().numpy().astype(np.complex128), outs["b"].cpu().numpy().astype(np.complex128)
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
        byts = {"a": 8 * n + 8 * (n // M), "b": 24 * n + 8 * (n // M), "c": 8 * n + 8 * (n // M)}
        lo = {k: float(np.min(v)) for k, v in times.items()}
        hi = {k: float(np.max(v)) for k, v in times.items()}

        def apart(p, q):  # the two spreads do not overlap
            return hi[p] < lo[q] or hi[q] < lo[p]

        res["shapes"][f"{pair}_M{M}_L{L}"] = {
            "fused_vs_pair_rel_rms": rel,
            "median_ms": med,
            "min_ms": lo,
            "max_ms": hi,
            "GBps": {k: byts[k] / (med[k] * 1e-3) / 1e9 for k in med},
            "a_over_b": med["a"] / med["b"],
            "a_over_c": med["a"] / med["c"],
            "a_b_distinguishable": apart("a", "b"),
            "a_c_distinguishable": apart("a", "c"),
        }
        del ddc, nco, dec_b, dec_c, outs
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
