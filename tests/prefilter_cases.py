"""
The motif sets, sequences and cases of tests/test_gpu_prefilter_candidates.py and tests/test_gpu_fp64_from_candidates.py, and what each case
must put in front of the kernels (CONDITIONS, tallied on the model alone: tests/test_prefilter_model_host.py asserts them without a GPU, the
GPU tests on what they compared).  Everything is seeded: a case is the same bytes wherever it is built.

Motif sets (log-odds of seeded position probabilities against a flat background, cutoffs as fractions of the best score):
    pair    72 motifs of 1 ... 15 columns (each width four times, 1 / 7 / 8 / 15 seven times): paired rows of one and two half-blocks, more
            than one paired row tile on both strands
    plain   40 motifs of 16 ... 31 columns (16 / 23 / 24 / 31 four times): plain rows of two k-blocks
    narrow  pair + plain + the A-rich and the AC-repeat motifs that make the flood stretches flood (one of them the poly-A consensus whose
            windows hang over the input's end)
    wide    every second motif of narrow (a third of them would fit ONE paired row tile, of two half-blocks: the wide kernel would never run
            a paired row of one) + 22 motifs of 32 ... 63 columns (32 / 47 / 48 / 63 among them): plain rows of three and four k-blocks --
            and one of 64 columns, which no row holds: it takes the all-fp64 path and must appear in no record
    small / small_wide   at most 6 table groups, for the long inputs
    alln    narrow with one 10-column motif at cutoff 0.0: a window of non-ACGT bases only scores 0 and is a hit, so the plan has
            alln_can_hit and the kernel may not drop such windows unseen
Plain rows of ONE k-block hold no motif of any plan the product builds (a motif of <= 15 columns rides a paired row): the `nopair` cases reach
f6_class<1> / f6_class2<1> through the measurement switch MS_PF_PAIR=0, which plans the narrow motifs on plain rows.
"""
import functools

import numpy as np

import prefilter_model as pm

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
N_RUNS = (1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 300)
N_PHASES = (0, 1, 31, 32, 63, 64, 127)
EDGE_RUNS = (31, 32, 33, 63, 64, 65)           # the lengths around a dead window of 32 / 64 bases: at every phase
TAIL_PREFIXES = (1, 31, 64, 65, 127, 128, 129, 1023, 1025)


# ------------------------------------------------------------------------------------------------------------------- motifs --

def _motif(rng, w, bias_to=None, sharp=0.0):
    p = rng.dirichlet(0.4 * np.ones(4), size=w).T
    if bias_to is not None:                                    # a consensus of our choosing, the other bases as they fell
        for c, b in enumerate(bias_to):
            p[:, c] *= 1.0 - sharp
            p[b, c] += sharp
    p = (p + 0.02) / 1.08
    return np.log2(p / 0.25)


def _rich(rng, word, w):
    """a motif whose consensus repeats `word` (A: poly-A; AC: the dinucleotide repeat)"""
    return _motif(rng, w, ["ACGT".index(word[c % len(word)]) for c in range(w)], sharp=0.8)


def _cutoff(w):
    return 0.92 if w <= 3 else (0.85 if w <= 7 else 0.78)


@functools.lru_cache(maxsize=None)
def motif_set(name):
    """(matrices, cutoffs) of a set"""
    rng = np.random.default_rng(4711)
    pair = [_motif(rng, w) for w in list(range(1, 16)) * 4 + [1, 7, 8, 15] * 3]
    plain = [_motif(rng, w) for w in list(range(16, 32)) * 2 + [16, 23, 24, 31] * 2]
    rich = [_rich(rng, "A", w) for w in (3, 6, 12, 14, 20, 28)] + [_rich(rng, "AC", w) for w in (5, 10, 24)]
    wide_only = [_motif(rng, w) for w in [32, 47, 48, 63] + list(range(33, 64, 2))] + [_rich(rng, "A", 40), _rich(rng, "A", 56)]
    w64 = _motif(rng, 64)
    narrow = pair + plain + rich
    if name in ("narrow", "alln"):
        mats = list(narrow)
    elif name == "wide":
        mats = narrow[::2] + rich[1::2]
        for w in (1, 7, 8, 15, 16, 23, 24, 31):                # every edge width of the narrow sets stays
            if not any(m.shape[1] == w for m in mats):
                mats.append([m for m in narrow if m.shape[1] == w][0])
        mats += wide_only + [w64]
    elif name == "small":
        mats = [pair[0], pair[6], pair[7], pair[14], rich[1], rich[2], plain[0], plain[7], plain[15], rich[4]]
    elif name == "small_wide":
        mats = [pair[0], pair[7], rich[2], wide_only[0], wide_only[3]]
    else:
        raise KeyError(name)
    cut = np.array([_cutoff(m.shape[1]) for m in mats])
    if name == "alln":
        at = [i for i, m in enumerate(mats) if m.shape[1] == 10][0]
        cut[at] = 0.0
    return mats, cut


def flat(mats):
    return np.concatenate([m.ravel() for m in mats]), np.array([m.shape[1] for m in mats], dtype=np.int32)


def consensus(m):
    return "".join("ACGT"[b] for b in m.argmax(axis=0))


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


# ---------------------------------------------------------------------------------------------------------------- sequences --

def _spacer(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def _plants(rng, mats):
    """every motif's consensus and its reverse complement between random spacers of 2 ... 9 bases"""
    out = []
    for m in mats:
        c = consensus(m)
        out += [c, _spacer(rng, int(rng.integers(2, 10))), revcomp(c), _spacer(rng, int(rng.integers(2, 10)))]
    return "".join(out)


def _n_runs(rng, at):
    """runs of N of every length of N_RUNS, the lengths of EDGE_RUNS at every phase of N_PHASES and the others at one each, every run on its
    phase mod 128 behind at least two spacer bases; `at`: the position the text starts at"""
    todo = [(n, p) for n in EDGE_RUNS for p in N_PHASES] + [(n, N_PHASES[i % len(N_PHASES)]) for i, n in enumerate(N_RUNS) if n not in EDGE_RUNS]
    out = []
    while todo:
        pad = lambda it: (it[1] - (at + 2)) % 128 + 2
        nxt = min(todo, key=pad)
        todo.remove(nxt)
        out += [_spacer(rng, pad(nxt)), "N" * nxt[0]]
        at += pad(nxt) + nxt[0]
    return "".join(out)


def _floods(rng, extra):
    f = ["A" * 300, "T" * 300, "AC" * 150]
    if extra:
        f += ["A" * 77, "T" * 131, "CA" * 100, "A" * 200, "GT" * 90, "T" * 260, "A" * 333, "T" * 415, "AC" * 120, "A" * 290, "T" * 190, "TG" * 110, "A" * 401, "T" * 350,
              "CA" * 64, "A" * 129, "T" * 255]
    return "".join(x + _spacer(rng, int(rng.integers(3, 40))) for x in f)


@functools.lru_cache(maxsize=None)
def sequence(set_name, kind="full", fill_to=0):
    """full: plants (the text starts with them: the tail cases take prefixes), flood stretches, a few IUPAC letters and lower case, the runs of
    N, one 128-aligned stretch of N only (256 bases: a whole double pass of dead windows), sparse background, and a poly-A end, so that
    windows hanging over the input's end flag.  flood: more and odder flood stretches.  fill_to: background with an occasional run of N and
    poly-A stretch up to that many bases, for the inputs that must be long."""
    rng = np.random.default_rng(977)
    mats, _ = motif_set(set_name)
    s = _plants(rng, mats) + _floods(rng, kind == "flood")
    s += "ACGRTYACKGTMacgtnacgwSACGTBDHVacgu" + _spacer(rng, 20)
    s += _n_runs(rng, len(s))
    s += _spacer(rng, (-len(s) - 2) % 128 + 2) + "N" * 256
    s += _spacer(rng, 600)
    while len(s) < fill_to - 200:
        s += _spacer(rng, 4000) + "N" * 40 + _spacer(rng, 300) + "A" * 150
    s = s[:max(fill_to - 150, 0)] if fill_to else s
    return s + "A" * 150


# -------------------------------------------------------------------------------------------------------------------- cases --

KERNELS = {                     # kernel -> (motif set, MS_PF_DENSE, geom's wide, dense)
    "parked": ("narrow", "0", 0, 0),
    "dense": ("narrow", "1", 0, 1),
    "wide": ("wide", "0", 1, 0),
}


def counter_point(blocks, pass_windows):
    """launch_shape (ms_scan_geom.cpp) hands a wave one even unit, without the counters, while the input's passes are at most
    8 x max(wave_passes, 8) x waves -- wave_passes is 2 there for inputs this short: 64 passes per wave, 16 waves per block.  Returns the
    largest such input in bases."""
    return 64 * 16 * blocks * pass_windows


def _case(kind, kernel, strand=3, set_name=None, seq=("full", 0), prefix=None, env=None, budget=70 * 1024, pair=True, expect=None):
    base_set, dense, wide, is_dense = KERNELS[kernel]
    e = {"MS_PF_DENSE": dense}
    e.update(env or {})
    if not pair:
        e["MS_PF_PAIR"] = "0"
    x = {"wide": wide, "dense": is_dense, "pass_windows": 64 if wide else 128}
    x.update(expect or {})
    return {"kind": kind, "kernel": kernel, "strand": strand, "set": set_name or base_set, "seq": seq, "prefix": prefix, "env": e, "budget": budget,
            "pair": pair, "expect": x}


def _cases():
    c = {}
    for k in KERNELS:
        for strand in (1, 2, 3):
            c[f"basic-{k}-s{strand}"] = _case("basic", k, strand)
        for n in TAIL_PREFIXES:
            c[f"tail-{k}-{n}"] = _case("tail", k, prefix=n)
    for k in ("parked", "wide"):
        c[f"parking-{k}-cap16"] = _case("parking", k, seq=("flood", 0), env={"MS_PF_RARE_CAP": "16"}, expect={"rare_cap": 16})
        c[f"parking-{k}-default"] = _case("parking", k, seq=("flood", 0))
        for blocks in (1, 3):
            n = counter_point(blocks, 64 if k == "wide" else 128) + 257
            c[f"counter-{k}-b{blocks}"] = _case("counter", k, set_name="small_wide" if k == "wide" else "small", seq=("full", n),
                                                env={"MS_PF_MAX_BLOCKS": str(blocks)}, expect={"counter_used": 1, "blocks_per_tile": blocks})
        c[f"tiles-{k}"] = _case("tiles", k, env={"MS_PF_LDS_BUDGET": "16384"}, budget=16384)
        c[f"nopair-{k}"] = _case("nopair", k, pair=False)
    for k in ("parked", "dense"):
        c[f"alln-{k}"] = _case("alln", k, set_name="alln", expect={"skip_alln": 0})
    return c


CASES = _cases()

# what a case of a kind must hold, on the model alone (tally()); forms: (paired, instructions per row tile) the plan must have
CONDITIONS = {
    "basic": {"fields_flagging_all": 1, "residues": 128, "dead_windows": 100, "hanging_flags": 1},      # (hanging_flags: where the forward strand is scanned -- the pad reads as A)
    "tail": {},
    "parking": {"fields_flagging_all": 1, "residues": 128, "events_ge48": 100, "events_1_8": 100, "dead_windows": 100},
    "counter": {"fields_flagging_all": 1, "residues": 128, "dead_windows": 100},
    "tiles": {"fields_flagging_all": 1, "tiles": 2, "dead_windows": 100},
    "nopair": {"fields_flagging_all": 1, "residues": 128, "dead_windows": 100},
    "alln": {"fields_flagging_all": 1, "dead_windows": 100, "dead_flags": 100},
}
FORMS = {        # (set, both strands scanned) -> the row forms the plan holds: (paired, instructions per row tile).  One strand puts twice the motifs on a row tile
    ("narrow", True): {(1, 1), (1, 2), (0, 2)}, ("narrow", False): {(1, 1), (1, 2), (0, 2)},
    ("alln", True): {(1, 1), (1, 2), (0, 2)},
    ("wide", True): {(1, 1), (1, 2), (0, 2), (0, 3), (0, 4)}, ("wide", False): {(1, 2), (0, 2), (0, 4)},
    ("small", True): {(1, 2), (0, 2)},
    ("small_wide", True): {(1, 2), (0, 4)},
    ("nopair", "narrow"): {(0, 1), (0, 2)},
    ("nopair", "wide"): {(0, 1), (0, 2), (0, 3), (0, 4)},
}


def case_forms(case):
    return FORMS.get((case["kind"], case["set"])) or FORMS[case["set"], case["strand"] == 3]


def case_text(case):
    s = sequence(case["set"], *case["seq"])
    return s[:case["prefix"]] if case["prefix"] else s


def group_span(plan, wide_kernel):
    """per group: the bases a dead window is made of -- 64 in a tile with row tiles of 3 or 4 k-blocks under the wide kernel, else 32"""
    kb, tf = plan["group_kb"], plan["tile_first_group"]
    span = np.full(len(kb), 32, dtype=np.int64)
    for t in range(len(tf) - 1):
        if wide_kernel and kb[tf[t]:tf[t + 1]].max() > 2:
            span[tf[t]:tf[t + 1]] = 64
    return span


def expected_flags(plan, model, isn, wide_kernel, skip_alln):
    """(lower, upper): the device's flags must hold every bit of lower and no bit outside upper -- equal but in dead windows under skip_alln"""
    lower = model.copy()
    if skip_alln:
        span = group_span(plan, wide_kernel)
        for sp in np.unique(span):
            dead = pm.dead_windows(isn, int(sp))
            lower[np.ix_(span == sp, dead)] = 0
    return lower, model


def tally(plan, model, isn, case, widths):
    """what the case holds, from the plan and the model's flags alone"""
    L = model.shape[1]
    occ = pm.occupied_mask(plan)
    lower, _ = expected_flags(plan, model, isn, bool(case["expect"]["wide"]), True)
    t = {"forms": {(int(p > 0), int(k)) for p, k in zip(plan["group_paired"], plan["group_kb"])}, "tiles": int(plan["n_tiles"]),
         "groups": int(len(occ)), "empty_field_flags": int((model & ~occ[:, None]).any())}
    ever = np.bitwise_or.reduce(lower, axis=1) if L else np.zeros(len(occ), dtype=np.uint16)
    t["fields_flagging_all"] = int((ever == occ).all())
    t["residues"] = len(np.unique(np.nonzero(lower.any(axis=0))[0] % 128))
    t["dead_windows"] = int(pm.dead_windows(isn, 32).sum())
    t["dead_flags"] = int(np.count_nonzero(model & ~lower))
    hang = 0
    for q, n in zip(*np.nonzero(plan["group_fields"] >= 0)):
        w = int(widths[plan["group_fields"][q, n]])
        if w > 1 and L:
            hang += int(((model[q, max(L - w + 1, 0):] >> np.uint16(n)) & np.uint16(1)).sum())
    t["hanging_flags"] = hang
    ge48 = small = 0
    nb = (L + 31) // 32
    any_ = np.zeros((model.shape[0], nb * 32), dtype=bool)
    any_[:, :L] = lower != 0
    tiles = pm.row_tiles(plan)
    for q0 in sorted({q for q, _ in tiles}):
        n = sum(1 for q, _ in tiles if q == q0)
        halves = (any_[q0] | any_[q0 + 1], any_[q0 + 2] | any_[q0 + 3]) if n == 4 else (any_[q0], any_[q0 + 1])
        lanes = halves[0].reshape(nb, 32).sum(axis=1) + halves[1].reshape(nb, 32).sum(axis=1)
        ge48 += int((lanes >= 48).sum())
        small += int(((lanes >= 1) & (lanes <= 8)).sum())
    t["events_ge48"], t["events_1_8"] = ge48, small
    return t


_BUILT = {}


def build(case, _lib):
    """the case's motifs, text, plan and model flags (the model is kept per (set, strand, rows paired or not, text): cases that differ only in
    how the kernel is launched share it).  The caller has set the case's environment (the plan reads MS_PF_PAIR)."""
    mats, cut = motif_set(case["set"])
    vals, widths = flat(mats)
    text = case_text(case)
    pw = _lib.PwmSet(vals, widths, cut)
    plan = pw.plan(case["strand"], case["budget"])
    key = (case["set"], case["strand"], case["pair"], case["seq"], case["prefix"])
    if key not in _BUILT:
        codes, isn = pm.encode(text)
        _BUILT[key] = (codes, isn, pm.model_flags(plan, codes, isn))
    codes, isn, model = _BUILT[key]
    return {"mats": mats, "cutoffs": cut, "vals": vals, "widths": widths, "text": text, "pwms": pw, "plan": plan, "codes": codes, "isn": isn,
            "model": model}


def unmet(case, t):
    """the conditions of the case's kind that its tally misses (empty: all met)"""
    bad = [f"{k}: {t[k]} < {v}" for k, v in CONDITIONS[case["kind"]].items() if t[k] < v and not (k == "hanging_flags" and case["strand"] == 2)]
    if t["forms"] != case_forms(case):
        bad.append(f"row forms {sorted(t['forms'])}, the case claims {sorted(case_forms(case))}")
    if t["empty_field_flags"]:
        bad.append("the model flags an empty field")
    if case["set"].startswith("small") and t["groups"] > 6:
        bad.append(f"{t['groups']} groups in a small set")
    return bad
