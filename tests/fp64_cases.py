"""
The cases of tests/test_gpu_fp64_from_candidates.py: region sets of at most 10 000 bases for the motif sets `narrow` and `wide` of
prefilter_cases, with regions of 0, 1, W - 1, W and W + 1 bases back to back among ordinary ones (W the width of a motif whose consensus the
W-base region is) and a run of tiny regions (three region starts within 64 bases: the fp64 kernels' find_region path), and `polya`: poly-A
regions under a few poly-A motifs, where a chunk of the all-flagged list yields more hits than the fp64 stage's hit stage holds.
CONDITIONS: what a set must hold, tallied from the oracle and the model alone (tests/test_prefilter_model_host.py).
"""
import os
import re

import numpy as np

import prefilter_cases as pc
import prefilter_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT_STAGE = 2048                      # kHitStage / RwStage (ms_fp64.hip): hits a block stages between two flushes
SETS = {"narrow": (1, 8, 15, 16, 31), "wide": (1, 15, 16, 31, 32, 63, 64), "polya": ()}     # the widths W whose regions of W - 1, W, W + 1 bases the set holds
CONDITIONS = {
    "narrow": {"exact_fit_hits": 5, "tiny_run": 30, "flags_across_ends": 100, "empty_regions": 2, "one_base_regions": 2},
    "wide": {"exact_fit_hits": 7, "tiny_run": 30, "flags_across_ends": 100, "empty_regions": 2, "one_base_regions": 2, "exact_path_hits": 1},
    "polya": {"hits_of_fullest_chunk": HIT_STAGE + 1},
}


def rw_chunk_from_source():
    """kRwChunk as ms_fp64.hip defines it (the library reports its own copy in ms_debug_scan_candidates' geom: the GPU test compares)"""
    text = open(os.path.join(ROOT, "motifscan_amd", "csrc", "ms_fp64.hip")).read()
    threads, per = (int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("kRwThreads", "kRwPerThread"))
    assert re.search(r"constexpr int kRwChunk = kRwThreads \* kRwPerThread;", text)
    return threads * per


def _regions(name):
    rng = np.random.default_rng(31)
    if name == "polya":
        mats = [pc._rich(np.random.default_rng(8), "A", w) for w in (6, 8, 10, 12)]
        return mats, np.full(4, 0.8), ["A" * 500] * 20
    mats, cut = pc.motif_set(name)
    text = pc._plants(rng, mats) + "A" * 100 + pc._spacer(rng, 7) + "T" * 90 + "ACGRTYNNNNNacgtn" + pc._spacer(rng, 30) + "N" * 40 + pc._spacer(rng, 50)
    regs, at = [], 0
    while at < len(text):
        n = int(rng.integers(300, 500))
        regs.append(text[at:at + n])
        at += n
    special = ["", "A"]
    for w in SETS[name]:
        c = pc.consensus([m for m in mats if m.shape[1] == w][0])
        special += [c[:-1], c, c + "A", pc.revcomp(c), "C" + c]
    tiny = [("ACGT" * 2)[i % 5:i % 5 + i % 4] for i in range(44)]          # 0 ... 3 bases each
    half = len(regs) // 2
    return mats, cut, regs[:half] + special + regs[half:] + tiny + ["", "A", pc._spacer(rng, 200) + "A" * 40]


_BUILT = {}


def build(name, _lib, oracle, strand=3):
    """dict(vals, widths, cutoffs, raw, offsets, strand, plan, oracle, codes, isn, model, pwms args) of a set"""
    if (name, strand) in _BUILT:
        return _BUILT[name, strand]
    mats, cut, regs = _regions(name)
    vals, widths = pc.flat(mats)
    raw = "".join(regs)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in regs])]).astype(np.int64)
    plan = _lib.PwmSet(vals, widths, cut).plan(strand)
    codes, isn = pm.encode(raw)
    case = {"name": name, "vals": vals, "widths": widths, "cutoffs": np.asarray(cut, dtype=np.float64), "raw": raw.encode(), "offsets": offsets,
            "strand": strand, "plan": plan, "codes": codes, "isn": isn, "model": pm.model_flags(plan, codes, isn)}
    case["oracle"] = oracle.scan_arrays(vals, widths, case["cutoffs"], case["raw"], offsets, strand, 4)
    _BUILT[name, strand] = case
    return case


def all_flagged(case):
    """every occupied field flagged at every base: uint16 [n_groups, n_bases]"""
    occ = pm.occupied_mask(case["plan"])
    return np.repeat(occ[:, None], int(case["offsets"][-1]), axis=1)


def flags_of(records, case):
    return pm.decode_records(records, case["plan"]["group_fields"].shape[0], int(case["offsets"][-1]))[0]


def tally(case, oracle):
    off, want, widths = case["offsets"], case["oracle"], case["widths"]
    lens = np.diff(off)
    motif = np.repeat(np.arange(len(widths)), np.diff(want["motif_offsets"]))
    t = {"bases": int(off[-1]), "empty_regions": int((lens == 0).sum()), "one_base_regions": int((lens == 1).sum()),
         "exact_fit_hits": len({int(w) for w in widths[motif][lens[want["seq_idx"]] == widths[motif]]}),
         "exact_path_hits": int(np.isin(motif, case["plan"]["exact_motifs"]).sum())}
    small = (lens <= 3).astype(int)
    run = best = 0
    for s in small:
        run = run + 1 if s else 0
        best = max(best, run)
    t["tiny_run"] = best
    # flagged windows that run past their region's end: what the fp64 stage must drop
    region_of = np.repeat(np.arange(len(lens)), lens)
    room = off[region_of + 1] - np.arange(int(off[-1]))
    across = 0
    gf = case["plan"]["group_fields"]
    for q, n in zip(*np.nonzero(gf >= 0)):
        across += int((((case["model"][q] >> np.uint16(n)) & np.uint16(1)).astype(bool) & (room < widths[gf[q, n]])).sum())
    t["flags_across_ends"] = across
    rec = pm.pack_records(all_flagged(case)) if case["name"] == "polya" else []        # (the other sets make no claim about it)
    chunk = rw_chunk_from_source()
    best = 0
    for c in range(0, len(rec), chunk):
        got = pm.hits_from_candidates(oracle, case, flags_of(rec[c:c + chunk], case))
        best = max(best, int(got["motif_offsets"][-1]))
    t["hits_of_fullest_chunk"] = best
    return t


def unmet(name, t):
    bad = [f"{k}: {t[k]} < {v}" for k, v in CONDITIONS[name].items() if t[k] < v]
    if t["bases"] > 10000:
        bad.append(f"{t['bases']} bases")
    return bad
