"""
The integer pre-filter as a numpy model, and the candidate list as the model sees it -- shared by the CPU proof that the plan never loses a
reference hit (tests/test_host_cabi.py), the checks of the model and of the GPU cases' conditions (tests/test_prefilter_model_host.py), and the
GPU tests that hold prefilter_f6_kernel and the fp64 stage to it record by record (tests/test_gpu_prefilter_candidates.py,
tests/test_gpu_fp64_from_candidates.py).

The object modelled is the PHYSICAL fp6 operand image the kernel reads, decoded by ms_debug_plan_rows (_lib.PwmSet.plan): a table group has
16 fields, a field's accumulator at window start g is

    acc = bias + sum over the columns c < group_cols - 1 of (base g + c is non-ACGT ? 0 : rows[group][field][c][code of base g + c])

in units of 1/8, and the field is a candidate at g iff acc >= 0.  The group's last column carries the bias and is never cleared.  Codes and
non-ACGT bits past the set's end are zero, as the pad words behind the packed planes are.  A candidate record is g << 30 | group << 16 | flags,
bit n of the flags = field n; 0 is an empty slot (cand_pack, emit_rec).
"""
import numpy as np

LUT = {c: i for i, c in enumerate("ACGT")}
_PAD = 70              # bases past the end a window can reach (63 columns), and a little more


def encode(seq):
    """2-bit codes and the non-ACGT mask of a sequence, as convert_seq sees it (cscore.c:92-111: case folded, the rest 'adds nothing')."""
    up = seq.upper()
    codes = np.array([LUT.get(c, 0) for c in up], dtype=np.int64)
    isn = np.array([c not in LUT for c in up], dtype=bool)
    return codes, isn


def _code5(codes, isn):
    """codes with 4 for a non-ACGT base, padded with A (code 0, not N) past the end"""
    c5 = np.where(np.asarray(isn, dtype=bool), 4, np.asarray(codes)).astype(np.int8)
    return np.concatenate([c5, np.zeros(_PAD, dtype=np.int8)])


def _tab5(plan, q):
    """rows of group q as [16 fields][columns][5]: what a base adds, with a zero entry for a non-ACGT base"""
    r = plan["rows"][q].astype(np.int32)
    return np.concatenate([r, np.zeros(r.shape[:2] + (1,), dtype=np.int32)], axis=2)


def model_acc(plan, codes, isn, q, n, g):
    """the accumulator of field n of group q at window start g (the failure messages name it)"""
    c5 = _code5(codes, isn)
    tab = _tab5(plan, q)[n]
    ncol = int(plan["group_cols"][q]) - 1
    return int(plan["bias"][q, n]) + int(sum(tab[c, c5[g + c]] for c in range(ncol)))


def model_flags(plan, codes, isn):
    """uint16 [n_groups, L]: bit n of [q, g] = field n of group q is a candidate at window start g.  The 16 fields of a group go through
    numpy together: one gather of [16, L] per column that adds anything."""
    L = len(codes)
    c5 = _code5(codes, isn)
    n_groups = plan["group_fields"].shape[0]
    out = np.zeros((n_groups, L), dtype=np.uint16)
    weight = (1 << np.arange(16)).astype(np.uint16)[:, None]
    for q in range(n_groups):
        ncol = int(plan["group_cols"][q]) - 1                   # the last column of the group's fields carries the bias
        tab = _tab5(plan, q)
        assert not tab[:, ncol:, :].any()
        acc = np.repeat(plan["bias"][q].astype(np.int32)[:, None], L, axis=1)
        for c in range(ncol):
            if tab[:, c, :].any():
                acc += tab[:, c, :][:, c5[c:c + L]]
        out[q] = ((acc >= 0) * weight).sum(axis=0, dtype=np.uint16)
    return out


def occupied_mask(plan):
    """uint16 [n_groups]: bit n = field n of the group holds a motif"""
    return ((plan["group_fields"] >= 0) * (1 << np.arange(16))).sum(axis=1).astype(np.uint16)


def pack_records(flags):
    """one record per (g, group) with a flag set, in (group, g) order"""
    q, g = np.nonzero(flags)
    return (g.astype(np.uint64) << np.uint64(30)) | (q.astype(np.uint64) << np.uint64(16)) | flags[q, g].astype(np.uint64)


def decode_records(records, n_groups, L):
    """(flags uint16 [n_groups, L], tally): the array model_flags returns, from a flat record list, and what of the list does not belong in
    one -- tally = dict(empty, bad_g, bad_group, repeated): empty slots, records with g >= L, with group >= n_groups, and (g, group) pairs that
    came more than once (their flags are ORed)."""
    rec = np.asarray(records, dtype=np.uint64)
    live = rec[(rec & np.uint64(0xFFFF)) != 0]
    g = (live >> np.uint64(30)).astype(np.int64)
    q = ((live >> np.uint64(16)) & np.uint64(0x3FFF)).astype(np.int64)
    f = (live & np.uint64(0xFFFF)).astype(np.uint16)
    bad_g, bad_q = g >= L, q >= n_groups
    ok = ~bad_g & ~bad_q
    g, q, f = g[ok], q[ok], f[ok]
    flags = np.zeros((n_groups, L), dtype=np.uint16)
    np.bitwise_or.at(flags, (q, g), f)
    tally = {"empty": int(rec.size - live.size), "bad_g": int(bad_g.sum()), "bad_group": int((bad_q & ~bad_g).sum()),
             "repeated": int(g.size - np.unique(q * max(L, 1) + g).size)}
    return flags, tally


def dead_windows(isn, span):
    """bool [L]: the `span` bases from g on are all non-ACGT (bases past the end are not): the windows scan_pass / scan_pass2 drop unseen
    when no motif of the plan can report a window of non-ACGT bases only (PfArgs::skip_alln)"""
    n = np.concatenate([np.asarray(isn, dtype=np.int64), np.zeros(span, dtype=np.int64)])
    cs = np.concatenate([[0], np.cumsum(n)])
    return (cs[span:span + len(isn)] - cs[:len(isn)]) == span


def row_tiles(plan):
    """per group: (first group of its 32-row operand tile, lane half h of the group in it) -- a paired row tile is four groups (field X and Y
    of half 0, then of half 1), a plain one two"""
    paired = plan["group_paired"]
    out, q = [], 0
    while q < len(paired):
        n = 4 if paired[q] else 2
        out += [(q, (k >> 1) if paired[q] else k) for k in range(n)]
        q += n
    return out


def hits_from_candidates(oracle, case, flags):
    """What the fp64 stage must make of a candidate list whose flags are `flags` [n_groups, n_bases]: the oracle's all-motif scan of the case
    (case["oracle"], or computed here), of which a fast motif's hit stays iff its (motif, window start) is flagged -- with both strands
    scanned either strand's field keeps both strands' hits, the two being re-scored together -- and every hit of a motif on the all-fp64
    path stays.  In the reference's order.  case: dict(vals, widths, cutoffs, raw, offsets, strand, plan)."""
    want = case.get("oracle")
    if want is None:
        want = oracle.scan_arrays(case["vals"], case["widths"], case["cutoffs"], case["raw"], case["offsets"], case["strand"], 4)
    plan, P = case["plan"], len(case["widths"])
    offsets = np.asarray(case["offsets"], dtype=np.int64)
    n_bases = int(offsets[-1])
    flagged = np.zeros((P, max(n_bases, 1)), dtype=bool)
    for q, n in zip(*np.nonzero(plan["group_fields"] >= 0)):
        flagged[plan["group_fields"][q, n]] |= ((flags[q] >> np.uint16(n)) & np.uint16(1)).astype(bool)
    flagged[plan["exact_motifs"]] = True
    motif = np.repeat(np.arange(P), np.diff(want["motif_offsets"]))
    keep = flagged[motif, offsets[want["seq_idx"]] + want["pos"]]
    out = {k: want[k][keep] for k in ("seq_idx", "pos", "score", "strand")}
    out["motif_offsets"] = np.concatenate([[0], np.cumsum(np.bincount(motif[keep], minlength=P))]).astype(np.int64)
    return out
