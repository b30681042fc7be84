#!/usr/bin/env python3
"""
tools/sitesignal_time.py -- device time of ms_result_site_signal ("Signal tracks over sites") on the result of one
block of the benchmark's region set, beside ms_result_site_base_counts on the same result in the same process as the yardstick.

    python tools/sitesignal_time.py [--regions 125000] [--length 500] [--motifs 579] [--repeats 5] [--out FILE]

One process, one scan (p = 1e-4, both strands, de-duplicated), one synthetic track (a seeded int32 per base).  Per flank (0, 64, 256)
and per output selection (profile only, per_site only, both): one warm call, then the median over --repeats calls of the call's
device_ms (HIP events on the library's stream, first launch -> last kernel done).  The outputs live in device memory, so no call waits
for a copy of the per-site array.  The byte floor of a flank is sites x (W + 2 * flank) x 4 B, summed per motif, over the HBM rate a
streaming read reaches on this device (6.3 TB/s): what the track's values alone would cost if every site read them from HBM once.  The
profile and the per-site sums are checked against each other (the core columns of a motif's profile sum to its sites' core sums).
Prints one JSON line, and writes it to --out.  Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motifscan_amd import _lib, synth  # noqa: E402

HBM_TBPS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=125000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--flanks", default="0,64,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("sitesignal_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    import torch
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(a.motifs, p_value="1e-4")
    bases, offsets = synth.make_regions(a.regions, a.length, seed=1)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(bases, offsets)
    values = np.random.default_rng(2).integers(0, 50, size=int(offsets[-1]), dtype=np.int64).astype(np.int32)
    tr = _lib.Track.from_values(values, offsets)
    res = _lib.scan(pw, sq, 3).dedup(pw)
    n_hits, P = res.n_hits, len(widths)
    per_motif = np.diff(res.motif_offsets)
    times, floors, all_ms = {}, {}, {}
    for flank in [int(f) for f in a.flanks.split(",")]:
        C = int(widths.max()) + 2 * flank
        d_sum, d_cov = (torch.zeros((P, 2, C), dtype=torch.int64, device="cuda") for _ in range(2))
        d_n = torch.zeros((P, 2), dtype=torch.int64, device="cuda")
        d_ps = torch.zeros((n_hits, 3), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ptr = [int(t.data_ptr()) for t in (d_sum, d_cov, d_n, d_ps)]
        for mode, kw in (("profile", dict(per_site=False, out=(ptr[0], ptr[1], ptr[2], None))),
                         ("per_site", dict(profile=False, per_site=True, out=(None, None, ptr[2], ptr[3]))),
                         ("both", dict(per_site=True, out=tuple(ptr)))):
            ms = []
            for _ in range(1 + a.repeats):
                res.site_signal(pw, tr, flank, **kw)
                ms.append(res.site_signal_ms)
            times[f"flank{flank}_{mode}"] = statistics.median(ms[1:])
            all_ms[f"flank{flank}_{mode}"] = ms
        torch.cuda.synchronize()
        total, n_sites, ps = d_sum.cpu().numpy(), d_n.cpu().numpy(), d_ps.cpu().numpy()
        if int(n_sites.sum()) != n_hits:
            raise SystemExit("n_sites does not sum to the number of hits")
        core = np.add.reduceat(ps[:, 1], res.motif_offsets[:-1][per_motif > 0])
        prof = np.array([total[m, :, flank:flank + int(widths[m])].sum() for m in range(P)])[per_motif > 0]
        if not np.array_equal(core, prof):
            raise SystemExit("the per-site core sums and the profile's core columns disagree")
        n_bytes = int((per_motif * (widths.astype(np.int64) + 2 * flank)).sum()) * 4
        floors[f"flank{flank}"] = {"track_bytes": n_bytes, "floor_ms": n_bytes / (HBM_TBPS * 1e12) * 1e3}
        del d_sum, d_cov, d_n, d_ps
    stack = []
    for _ in range(1 + a.repeats):
        res.site_base_counts(pw, sq, 64)
        stack.append(res.site_base_counts_ms)
    res.close()
    tr.close()
    sq.close()
    pw.close()
    line = json.dumps({"device": _lib.device_name(), "regions": a.regions, "length": a.length, "motifs": P, "strands": 2, "p_value": "1e-4",
                       "deduped": True, "n_hits": n_hits, "mean_width": float(np.mean(widths)), "track_values": int(offsets[-1]),
                       "site_signal_device_ms": times, "byte_floor": floors, "hbm_tbps_assumed": HBM_TBPS,
                       "site_base_counts_flank64_device_ms": statistics.median(stack[1:]),
                       "site_signal_ms_all": all_ms, "site_base_counts_ms_all": stack})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
