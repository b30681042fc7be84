"""
Shared by tests/test_bipartite_host.py and tests/test_gpu_bipartite.py: PWMs, bipartite specs and regions at the smallest shapes at which
ms_scan_best_bipartite can go wrong, the definition of include/motifscan_amd.h as a scalar loop (one placement, one strand, one gap and
one addition at a time, in Python floats), and the planted case of the end-to-end tests.  No GPU and no library call in here; the tests
pass ms_debug_bipartite_dims in.
"""
import numpy as np

from dimodel_cases import random_dna, random_pwm, with_n
from motifscan_amd.bipartite import Bipartite

CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
HALF = "AGGTCA"


# ------------------------------------------------------------------------------------------------ the definition, one operation at a time

def scalar_max_raw(mat):
    """max_raw of a PWM: the column maxima, none below 0, added in column order."""
    out = 0.0
    for c in range(mat.shape[1]):
        out += max(0.0, float(mat[:, c].max()))
    return out


_SUMS = {}                                                # (id(matrix), seq) -> (matrix, [(F(p), R(p))]): the specs and masks share them


def scalar_element_sums(mat, seq):
    """[(F(p), R(p))] for p = 0 .. L - W: columns in order, forward M[x][c], reverse M[3 - x][W - 1 - c]; a non-ACGT base adds nothing."""
    key = (id(mat), seq)
    if key not in _SUMS:
        W, rows, out = mat.shape[1], mat.tolist(), []
        for p in range(len(seq) - W + 1):
            fwd = rev = 0.0
            for c in range(W):
                x = CODE.get(seq[p + c])
                if x is not None:
                    fwd += rows[x][c]
                    rev += rows[3 - x][W - 1 - c]
            out.append((fwd, rev))
        _SUMS[key] = (mat, out)
    return _SUMS[key][1]


def scalar_scorable(mats, spec):
    for m in (mats[spec.a], mats[spec.b]):
        if any(v != v or v == float("inf") for v in m.ravel().tolist()):
            return False
    d = scalar_max_raw(mats[spec.a]) + scalar_max_raw(mats[spec.b])
    return d == d and d not in (float("inf"), float("-inf")) and d > 0.0


def scalar_best(mats, spec, seq, mask):
    """(score, pos, strand, gap) of one cell by the walk itself: p ascending, '+' before '-', g ascending, replace iff greater."""
    if not scalar_scorable(mats, spec):
        return np.nan, -1, 0, -1
    ma, mb = mats[spec.a], mats[spec.b]
    Wa, Wb, L = ma.shape[1], mb.shape[1], len(seq)
    denom = scalar_max_raw(ma) + scalar_max_raw(mb)
    sa, sb = scalar_element_sums(ma, seq), scalar_element_sums(mb, seq)
    best, where = -np.inf, (-1, 0, -1)
    for p in range(L - (Wa + spec.gap_min + Wb) + 1):
        for s in (1, 2):
            if not mask & s:
                continue
            for g in range(spec.gap_min, spec.gap_max + 1):
                if p + Wa + g + Wb > L:
                    break
                if s == 1:
                    raw = sa[p][0] + sb[p + Wa + g][1 if spec.flip else 0]
                else:
                    raw = sb[p][0 if spec.flip else 1] + sa[p + Wb + g][1]
                if raw / denom > best:
                    best, where = raw / denom, (p, s, g)
    return (best if where[1] else np.nan), where[0], where[1], where[2]


def scalar_planes(mats, specs, seqs, mask):
    shape = (len(specs), len(seqs))
    score, pos = np.full(shape, np.nan), np.full(shape, -1, dtype=np.int32)
    strand, gap = np.zeros(shape, dtype=np.int8), np.full(shape, -1, dtype=np.int16)
    for k, sp in enumerate(specs):
        for r, s in enumerate(seqs):
            score[k, r], pos[k, r], strand[k, r], gap[k, r] = scalar_best(mats, sp, s, mask)
    return score, pos, strand, gap


def same_planes(got, want):
    """Byte for byte: NaN where NaN, the same bits elsewhere, and the no-winner values whole."""
    (gs, gp, gd, gg), (ws, wp, wd, wg) = got, want
    assert gs.dtype == np.float64 and gp.dtype == np.int32 and gd.dtype == np.int8 and gg.dtype == np.int16
    assert gs.shape == ws.shape and np.array_equal(gp, wp) and np.array_equal(gd, wd) and np.array_equal(gg, wg)
    assert np.array_equal(np.isnan(gs), np.isnan(ws)) and np.array_equal(gs.view(np.int64)[~np.isnan(ws)], ws.view(np.int64)[~np.isnan(ws)])
    assert np.all(gp[np.isnan(gs)] == -1) and np.all(gd[np.isnan(gs)] == 0) and np.all(gg[np.isnan(gs)] == -1)


# ------------------------------------------------------------------------------------------------ matrices, specs, regions

def consensus_pwm(word, hi=1.5, lo=-1.25):
    m = np.full((4, len(word)), lo)
    for c, ch in enumerate(word):
        m[CODE[ch], c] = hi
    return m


# the matrices of world(): by name, so that a spec reads as what it is
M = {name: i for i, name in enumerate(("w1", "w2", "w3", "w31", "w32", "w33", "w34", "cap", "zero", "neg", "holes", "nan", "const", "half", "ca", "pinf"))}


def matrices(cap):
    mats = [random_pwm(w, 700 + w) for w in (1, 2, 3, 31, 32, 33, 34, cap)]
    mats.append(np.zeros((4, 1)))                          # every column zero: max_raw 0, legal beside a partner with max_raw > 0
    mats.append(-np.abs(random_pwm(4, 801)) - 0.5)         # every entry < 0: max_raw 0
    holes = random_pwm(5, 802)
    holes[0, 0] = holes[3, 4] = holes[2, 2] = -np.inf      # a window that starts with A (ends with A on '-') or holds G at column 2 sums to -inf
    mats.append(holes)
    bad = random_pwm(3, 803)
    bad[1, 1] = np.nan
    mats.append(bad)
    mats.append(np.tile(np.array([0.75, 0.5, 0.5, 0.75]), (4, 1)))        # column-constant, the columns a palindrome: F == R == 2.5 for every window
    mats.append(consensus_pwm(HALF))
    mats.append(consensus_pwm("CA"))
    pinf = random_pwm(2, 804)
    pinf[2, 0] = np.inf
    mats.append(pinf)
    assert len(mats) == len(M)
    return mats


def world_specs(G):
    m = M
    return [
        Bipartite(m["nan"], m["w1"], 0, 0, 2),                                                     # unscorable first
        Bipartite(m["w1"], m["w2"], 0, 0, 0), Bipartite(m["w2"], m["w1"], 1, 0, 0), Bipartite(m["w1"], m["w2"], 1, 7, 7),       # an element order that repeats
        Bipartite(m["w3"], m["w3"], 0, 3, 3), Bipartite(m["w3"], m["w3"], 1, 3, 3),                # a == b; with flip 1 '+' and '-' coincide
        Bipartite(m["w31"], m["w32"], 0, 0, 5), Bipartite(m["w33"], m["w34"], 1, 2, 2), Bipartite(m["w34"], m["w31"], 0, 30, 34),
        Bipartite(m["neg"], m["neg"], 0, 0, 1),                                                    # unscorable between: the sum of the max_raw is 0
        Bipartite(m["w1"], m["cap"], 0, 0, G), Bipartite(m["cap"], m["w1"], 1, 0, G), Bipartite(m["cap"], m["cap"], 0, 1, 1),
        Bipartite(m["w2"], m["pinf"], 0, 0, 1),                                                    # unscorable: a +inf entry
        Bipartite(m["half"], m["zero"], 0, 0, 0), Bipartite(m["zero"], m["half"], 1, 0, 3), Bipartite(m["neg"], m["half"], 0, 0, 2),
        Bipartite(m["holes"], m["w1"], 0, 0, 4), Bipartite(m["holes"], m["holes"], 1, 0, 2), Bipartite(m["w2"], m["holes"], 0, G, G),
        Bipartite(m["const"], m["const"], 0, 2, 5),
        Bipartite(m["half"], m["half"], 0, 1, 5), Bipartite(m["half"], m["ca"], 0, 0, 6), Bipartite(m["half"], m["half"], 1, 0, G),
        Bipartite(m["nan"], m["nan"], 1, 0, 0),                                                    # unscorable last
    ]


def span(mats, sp, g):
    return mats[sp.a].shape[1] + g + mats[sp.b].shape[1]


def n_regions(rng):
    """Non-ACGT bases around a HALF x{3} HALF site: in the spacer (ignored), inside either half (they add nothing), on the bases just
    outside; and at the 32-base word edges of a longer region."""
    site = HALF + "TTT" + HALF
    core = random_dna(rng, 5) + site + random_dna(rng, 6)
    out = [with_n(core, 11, 12, 13), with_n(core, 12), with_n(core, 7), with_n(core, 16), with_n(core, 5, 19), with_n(core, 4, 20), with_n(core, 5), with_n(core, 10, 14)]
    edge = random_dna(rng, 130)
    edge = edge[:20] + site + edge[35:]
    out += [with_n(edge, 31), with_n(edge, 32), with_n(edge, 63, 64), with_n(edge, 95), with_n(edge, 26, 27, 28)]
    out.append(with_n(random_dna(rng, 40), *range(0, 40, 2)))
    marked = bytearray((random_dna(rng, 60) + site + random_dna(rng, 60)).encode())
    marked[40:90] = bytes(marked[40:90]).lower()
    marked[100] = ord("R")
    out.append(marked.decode())
    return out


def tie_regions():
    """Regions in which placements tie: a homopolymer (every placement of the column-constant pair ties: pos 0, '+', g_min); HALF
    followed by CA at gaps 2 and 4 only (the smaller gap wins); the same HALF x{3} HALF site twice (the earlier position wins)."""
    return ["A" * 40, "TTTT" + HALF + "TTCACATTTTTTTT", "TTT" + HALF + "CCC" + HALF + "TTTTTTTT" + HALF + "CCC" + HALF + "TT"]


def short_regions(mats, specs, seed=20261021):
    """Lengths S - 1, S, S + 1 at the smallest and at the greatest gap of every spec (so that only some gaps fit), 63 / 64 / 65 placement
    starts of a few specs, the N placements, the tie regions, an empty region."""
    rng = np.random.default_rng(seed)
    lengths = set()
    for sp in specs:
        for g in (sp.gap_min, sp.gap_max):
            lengths |= {max(span(mats, sp, g) + d, 0) for d in (-1, 0, 1)}
    for sp in (specs[1], specs[6], specs[21]):
        lengths |= {span(mats, sp, sp.gap_min) - 1 + n for n in (63, 64, 65)}
    seqs = [random_dna(rng, n) for n in sorted(lengths)]
    seqs += n_regions(rng) + tie_regions() + ["", "G" * 30]
    return seqs


def planted_at(rng, length, sites):
    """A random region with the words of `sites` = [(start, word)] written into it."""
    b = bytearray(random_dna(rng, length).encode())
    for at, word in sites:
        b[at:at + len(word)] = word.encode()
    return b.decode()


def long_regions(mats, specs, seg, seed=5):
    """Lengths around a segment +- 1 and +- S, two and three segments; an N run across a segment (and word) edge; HALF x{g} HALF sites
    whose first half starts in the last window start of a segment (the second lies wholly in the next), whose second half straddles the
    edge, and one site in each of three segments in turn."""
    rng = np.random.default_rng(seed)
    sp = specs[21]                                         # HALF, HALF, flip 0, gaps 1 .. 5
    S = span(mats, sp, sp.gap_max)
    seqs = [random_dna(rng, n) for n in (seg - 1, seg, seg + 1, seg - S, seg + S, seg + S - 1, 2 * seg, 3 * seg)]
    n_run = bytearray(random_dna(rng, 2 * seg + 17).encode())
    n_run[seg - 9:seg + 12] = b"N" * 21
    seqs.append(n_run.decode())
    site = HALF + "CTC" + HALF
    seqs.append(planted_at(rng, 2 * seg + 40, [(seg - 1, site)]))                 # first half at the segment's last start
    seqs.append(planted_at(rng, 2 * seg + 40, [(seg - 12, site)]))                # second half straddles the edge: it starts at seg - 3
    seqs.append(planted_at(rng, 2 * seg + 40, [(seg - 15, site)]))                # the whole site ends on the segment's last base
    for k in range(3):
        seqs.append(planted_at(rng, 3 * seg - 5, [(k * seg + 100 + 7 * k, site)]))
    return seqs


def tile_specs(cap_index, other, n):
    """n specs of two cap-wide elements (four fill a tile to its last entry, the fifth opens the next) around a narrow one."""
    return [Bipartite(cap_index, cap_index, k & 1, k, k + 2) for k in range(n)] + [Bipartite(other, cap_index, 0, 0, 1)]


# ------------------------------------------------------------------------------------------------ the planted case

def planted_case(seed=7, n=200, length=100):
    """(inputs, controls, [half-site PWM]): n input regions that hold HALF, a spacer, HALF -- the spacers 1, 2, 4 and 5 in equal parts, so
    that the one length between them, 3, which the fixed-spacer comparison uses, is the length no site has --, and n control regions that
    hold the same two half-sites at least 24 bases apart, in an i.i.d. uniform background.  The PWM is the log-odds of the half-site."""
    rng = np.random.default_rng(seed)
    inputs, controls = [], []
    for i in range(n):
        g = (1, 2, 4, 5)[i % 4]
        at = int(rng.integers(0, length - (12 + g) + 1))
        inputs.append(planted_at(rng, length, [(at, HALF), (at + 6 + g, HALF)]))
    for i in range(n):
        d = int(rng.integers(24, length - 12 + 1))        # bases between the halves
        at = int(rng.integers(0, length - (12 + d) + 1))
        controls.append(planted_at(rng, length, [(at, HALF), (at + 6 + d, HALF)]))
    counts = np.ones((4, 6))
    for c, ch in enumerate(HALF):
        counts[CODE[ch], c] += 100
    return inputs, controls, [np.around(np.log(counts / counts.sum(axis=0) / 0.25), 5)]


PLANTED_SPEC = Bipartite(0, 0, 0, 1, 5)
PLANTED_FIXED = Bipartite(0, 0, 0, 3, 3)
