"""
Which share of a scan's hits order_finalize_kernel (csrc/ms_order.hip) would leave to order_overflow_kernel under a window of `tile` owned
slots and `ext` slots staged past them -- on the CPU, no GPU needed.

The benchmark's motif set is scanned with the oracle over i.i.d. regions at the benchmark's base frequencies (default 6000 x 500 bp); that
gives every motif's hits per region.  At L low key bits a run is one motif's hits in 2^(L - pbits - 1) regions (pbits = 9 for 500-bp regions),
so its length is taken as Poisson with mean (hits per region) x (regions per run).  A run of k hits that starts at slot s of its tile does
not close inside the window when s + k > tile + ext - 1, i.e. for max(0, k - ext) of the tile's `tile` start slots: the share of all hits
that stand in such runs is  sum_motifs sum_k P(k) k min(1, max(0, k - ext) / tile) / sum_motifs mean.

    python tools/order_window_share.py [--regions 6000] [--low-bits 16]
"""
import argparse
import os
import sys
from math import exp, lgamma, log

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from motifscan_amd import synth          # noqa: E402
from oracle import oracle                # noqa: E402


def poisson(k, m):
    return exp(k * log(m) - m - lgamma(k + 1)) if m > 0 else float(k == 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=6000)
    ap.add_argument("--low-bits", type=int, default=16)
    a = ap.parse_args()
    oracle.build()
    vals, widths, cutoffs = synth.load_motif_set(579)
    bases, offsets = synth.make_regions(a.regions, 500, seed=3)
    want = oracle.scan_arrays(vals, widths, cutoffs, bases.tobytes(), offsets, 3, os.cpu_count() or 1)
    per_region = np.diff(want["motif_offsets"]).astype(float) / a.regions
    lam = per_region * 2.0 ** (a.low_bits - 9 - 1)
    print(f"hits per (motif, region): {per_region.mean():.4f}; a million regions: {per_region.sum() * 1e6:.3g} hits")
    print(f"expected run at L = {a.low_bits}: mean over the motifs {lam.mean():.2f}, median {np.median(lam):.2f}, 99th percentile {np.percentile(lam, 99):.1f}, "
          f"busiest motif {lam.max():.1f} ({lam.max() / lam.mean():.0f} x the mean)")
    for tile, ext in ((960, 64), (896, 128), (1024, 256)):
        total = beyond = left = 0.0
        for m in lam:
            for k in range(1, 4000):
                p = poisson(k, m)
                if p < 1e-300 and k > m:
                    break
                total += k * p
                if k > ext:
                    beyond += k * p
                    left += k * p * min(1.0, (k - ext) / tile)
        print(f"window {tile} + {ext}: {beyond / total:.3g} of the hits stand in runs of more than {ext}; left to the overflow kernel: {left / total:.3g} of the hits")


if __name__ == "__main__":
    main()
