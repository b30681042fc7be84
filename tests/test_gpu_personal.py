"""
ms_genome_apply_alleles / ms_liftmap_* (ms_personal.hip) on the GPU against the sequential restatement personal.apply_alleles_host: the
output planes byte for byte (and the region hints, sizes, status and both lift maps at every position) for the hand-written cases, at
unit, chromosome, block and staging boundaries (ms_debug_personal_dims), for every source phase against every output phase, for dense
variants, any input order and seeded random cases; against the existing per-variant splice (ms_scan_alleles) and the reference
genome's own hits; the downstream entry points on the personal genome; and motifscan_amd.personal end to end.
"""
import ctypes

import numpy as np
import pytest

import personal_cases as pc
from motifscan_amd import _lib, personal, scanner

pytestmark = pytest.mark.gpu

ALL_PASS = -1e30


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


def seeded_matrix(width, seed):
    rng = np.random.default_rng(seed)
    ppm = rng.dirichlet(np.full(4, 0.4), size=width).T
    return np.round(np.log2((ppm + 0.01) / 1.04 / 0.25), 5)


def genome_of(chroms):
    return _lib.ResidentGenome({f"c{i}": s for i, s in enumerate(chroms)})


def host_planes(seq):
    """ms_pack_bases_host of a string"""
    units = (len(seq) + 31) // 32
    codes, nmask = np.zeros(2 * units, dtype=np.uint32), np.zeros(units, dtype=np.uint32)
    _lib.check(_lib.lib().ms_pack_bases_host(seq, len(seq), 1, _lib.ptr(codes, ctypes.c_uint32), _lib.ptr(nmask, ctypes.c_uint32)))
    return codes, nmask


def device_planes(genome, n_bases):
    """ms_genome_packed_host of a handle"""
    units = (n_bases + 31) // 32
    codes, nmask = np.zeros(2 * units, dtype=np.uint32), np.zeros(units, dtype=np.uint32)
    _lib.check(_lib.lib().ms_genome_packed_host(genome.h, _lib.ptr(codes, ctypes.c_uint32), _lib.ptr(nmask, ctypes.c_uint32)))
    return codes, nmask


def hint_arrays(n_bases):
    units, blocks = (n_bases + 31) // 32, (n_bases + 63) // 64 + 1
    return (np.zeros(2 * units, dtype=np.uint32), np.zeros(units, dtype=np.uint32), np.zeros(blocks, dtype=np.int32), np.zeros(4 * blocks, dtype=np.int32))


def check_planes(out, seqs):
    """Check 1: the planes are ms_pack_bases_host of the spliced string, and all four device arrays ms_debug_host_pack of it"""
    joined = b"".join(seqs)
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    assert [out.chrom_sizes[n] for n in out.names] == [len(s) for s in seqs]
    assert np.array_equal(out.offsets, offsets)
    nb = ctypes.c_int64()
    _lib.check(_lib.lib().ms_genome_size(out.h, None, ctypes.byref(nb)))
    assert nb.value == len(joined)
    got_c, got_n = device_planes(out, len(joined))
    want_c, want_n = host_planes(joined)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_n, want_n)
    want, got = hint_arrays(len(joined)), hint_arrays(len(joined))
    p = lambda a, t: _lib.ptr(a, t)
    u32, i32 = ctypes.c_uint32, ctypes.c_int32
    _lib.check(_lib.lib().ms_debug_host_pack(joined, p(offsets, ctypes.c_int64), len(seqs), p(want[0], u32), p(want[1], u32), p(want[2], i32), p(want[3], i32)))
    _lib.check(_lib.lib().ms_debug_seqset_planes(out.h, p(got[0], u32), p(got[1], u32), p(got[2], i32), p(got[3], i32)))
    for g, w, what in zip(got, want, ("codes", "nmask", "blk2reg", "blkinfo")):
        assert np.array_equal(g, w), what


def check_lifts(lm, want, chroms):
    """Check 8: every position 0 .. L and 0 .. L' of every chromosome, both directions, in ONE call each"""
    for key, lift, lens in (("to_alt", lm.to_alt, [len(s) for s in chroms]), ("to_ref", lm.to_ref, [len(s) for s in want["seqs"]])):
        ci = np.concatenate([np.full(n + 1, c, dtype=np.int32) for c, n in enumerate(lens)])
        ps = np.concatenate([np.arange(n + 1, dtype=np.int64) for n in lens])
        out, inside = lift(ci, ps)
        assert np.array_equal(out, np.concatenate([want[key][c][0] for c in range(len(lens))])), key
        assert np.array_equal(inside, np.concatenate([want[key][c][1] for c in range(len(lens))])), key + " inside"


def check_case(chroms, chrom, pos, ref, alt, check=None, skip=False, lifts=True, genome=None):
    """Checks 1, 6 and 8 of one call against the restatement; returns the restatement's result"""
    want = personal.apply_alleles_host(chroms, chrom, pos, ref, alt, refs_check=check, skip_mismatch=skip, lifts=lifts)
    g = genome if genome is not None else genome_of(chroms)
    n_in = sum(len(s) for s in chroms)
    before = device_planes(g, n_in)
    out, lm = _lib.apply_alleles(g, chrom, pos, [len(r) for r in ref], alt, refs=check, skip_mismatch=skip)
    try:
        check_planes(out, want["seqs"])
        assert np.array_equal(lm.status, want["status"]) and np.array_equal(lm.ref_mismatch, want["ref_mismatch"])
        assert (lm.n_chroms, lm.n_variants, lm.n_applied) == (len(chroms), len(pos), want["n_applied"])
        assert lm.ref_sizes.tolist() == [len(s) for s in chroms] and lm.alt_sizes.tolist() == want["sizes"].tolist()
        if lifts:
            check_lifts(lm, want, chroms)
        after = device_planes(g, n_in)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])      # the input genome is unchanged
    finally:
        out.close()
        lm.close()
        if genome is None:
            g.close()
    return want


# ------------------------------------------------------------------------------------------------ 1, 6: the hand-written cases on the device

@pytest.mark.parametrize("name", list(pc.CASES))
def test_hand_written_cases(name):
    case = pc.CASES[name]
    chrom, pos, ref, alt, check, skip = pc.case_args(case)
    want = check_case(case["chroms"], chrom, pos, ref, alt, check, skip)
    assert want["seqs"] == case["seqs"] and want["status"].tolist() == case["status"]


# ------------------------------------------------------------------------------------------------ 2: unit and chromosome edges, phases

EDGE_CHROMS = None


def edge_chroms():
    global EDGE_CHROMS
    if EDGE_CHROMS is None:
        rng = np.random.default_rng(21)
        EDGE_CHROMS = [pc.random_dna(rng, 77), b"", pc.random_dna(rng, 19), pc.random_dna(rng, 140)]
    return EDGE_CHROMS


@pytest.mark.parametrize("r", [0, 1, 2, 31, 32, 33, 65])
def test_unit_and_chromosome_edges(r):
    chroms = edge_chroms()
    rng = np.random.default_rng(100 + r)
    g = genome_of(chroms)
    L, n = len(chroms[3]), 0
    for x in (0, 31, 32, 33, 63, 64, L - 1, L):
        for a in (0, 1, 2, 31, 32, 33, 65):
            if x + r > L or r + a == 0:
                continue
            check_case(chroms, [3], [x], [chroms[3][x:x + r].decode()], [pc.random_dna(rng, a, 0.1).decode()], genome=g)
            n += 1
    assert n >= 20
    g.close()


def test_every_source_phase_against_every_output_phase():
    """A chain of variants on one chromosome built so that the genome piece behind variant k starts at source phase s and output phase o
    for every (s, o) of 32 x 32: r = 1 at the next x with (x + 1) % 32 == s, and a = (o - x - shift) % 32 alt bases."""
    rng = np.random.default_rng(5)
    pos, alt, shift, x = [], [], 0, 3
    for s in range(32):
        for o in range(32):
            x += 1
            while (x + 1) % 32 != s:
                x += 1
            a = (o - x - shift) % 32
            pos.append(x)
            alt.append(pc.random_dna(rng, a, 0.1).decode())
            shift += a - 1
    seq = pc.random_dna(rng, x + 50)
    ref = [seq[p:p + 1].decode() for p in pos]
    # the phases really are all there: source g + r, output g + r + the shift up to and including the variant
    got, shift = set(), 0
    for p, a in zip(pos, alt):
        shift += len(a) - 1
        got.add(((p + 1) % 32, (p + 1 + shift) % 32))
    assert len(got) == 1024
    want = check_case([seq], [0] * len(pos), pos, ref, alt, lifts=False)
    assert want["n_applied"] == 1024


# ------------------------------------------------------------------------------------------------ 3: dense variants

def test_dense_substitutions_and_deletions():
    rng = np.random.default_rng(7)
    chroms = [pc.random_dna(rng, 45), pc.random_dna(rng, 203), b""]
    L = len(chroms[1])
    comp = {ord("A"): "C", ord("C"): "G", ord("G"): "T", ord("T"): "A", ord("N"): "n"}
    # every base of a chromosome substituted: the genome pieces between are empty, a unit holds 32 alt pieces and 32 empty genome pieces
    want = check_case(chroms, [1] * L, list(range(L)), [chroms[1][x:x + 1].decode() for x in range(L)], [comp[chroms[1][x]] for x in range(L)])
    assert want["n_applied"] == L and want["seqs"][1] == bytes(ord(comp[b]) for b in chroms[1])
    # every second base deleted
    xs = list(range(0, L, 2))
    want = check_case(chroms, [1] * len(xs), xs, [chroms[1][x:x + 1].decode() for x in xs], [""] * len(xs))
    assert want["seqs"][1] == chroms[1][1::2]
    # ... and every base of the short chromosome replaced by two
    want = check_case(chroms, [0] * 45, list(range(45)), [chroms[0][x:x + 1].decode() for x in range(45)], ["GN"] * 45)
    assert want["seqs"][0] == b"GN" * 45


# ------------------------------------------------------------------------------------------------ 4: block and staging boundaries

def test_block_and_staging_boundaries():
    d = _lib.personal_dims()
    B, S = d["block_bases"], d["stage_variants"]
    rng = np.random.default_rng(9)
    long_len = 2 * B + 7
    chroms = [pc.random_dna(rng, 50), pc.random_dna(rng, 3 * B + 100), pc.random_dna(rng, 11)]
    # a block lies wholly inside one alt piece, and the blocks behind start their search in a piece that began blocks earlier
    want = check_case(chroms, [1], [B // 2 + 3], [""], [pc.random_dna(rng, long_len, 0.05).decode()], lifts=False)
    assert len(want["seqs"][1]) == len(chroms[1]) + long_len
    x = B // 2 + 3
    want = check_case(chroms, [1, 1, 2], [x, x + long_len + 40, 5], [chroms[1][x:x + long_len].decode(), "", "T"], ["", "ACGTN" * 9, "G"], lifts=False)
    assert len(want["seqs"][1]) == len(chroms[1]) - long_len + 45
    if S > 0:                                                    # S - 1, S and S + 1 variants whose pieces start inside ONE block (the second)
        for n in (S - 1, S, S + 1):
            xs = [B + 40 + 2 * i for i in range(n)]                # a substitution every other base: all of them in output block 1
            assert xs[-1] < 2 * B
            want = check_case(chroms, [1] * n, xs, [chroms[1][p:p + 1].decode() for p in xs], ["N" if i % 7 == 0 else "T" for i in range(n)], lifts=False)
            assert want["n_applied"] == n


# ------------------------------------------------------------------------------------------------ 5: order

def test_input_order_does_not_matter_beyond_the_index():
    chroms, chrom, pos, ref, alt = pc.random_case(77)
    rng = np.random.default_rng(3)
    V = len(pos)
    base = personal.apply_alleles_host(chroms, chrom, pos, ref, alt, refs_check=ref, skip_mismatch=True)
    g = genome_of(chroms)
    planes = None
    for trial in range(3):
        # a permutation that keeps the relative order of variants at one (chromosome, x): the index tie-break is then the same
        key = rng.random(V)
        same = {}
        for v in range(V):
            same.setdefault((chrom[v], pos[v]), []).append(v)
        perm = sorted(range(V), key=lambda v: (key[same[(chrom[v], pos[v])][0]], v))
        if trial == 0:
            perm = list(range(V))
        want = check_case(chroms, [chrom[v] for v in perm], [pos[v] for v in perm], [ref[v] for v in perm], [alt[v] for v in perm],
                          check=[ref[v] for v in perm], skip=True, genome=g)
        assert want["seqs"] == base["seqs"] and np.array_equal(want["status"], base["status"][perm])
    g.close()


@pytest.mark.parametrize("swap", [False, True])
def test_insertion_at_chromosome_end_and_variant_at_next_start(swap):
    """x = L_c of chromosome c and x = 0 of chromosome c + 1 are the SAME packed position: the key must still order by chromosome"""
    chroms = [b"ACGTACGTAC", b"GGGTTT", b"", b"CA"]
    items = [(0, 10, "", "TTT"), (1, 0, "G", "A"), (1, 6, "", "C"), (2, 0, "", "AAAA"), (3, 0, "", "G"), (1, 0, "", "NN")]
    if swap:
        items = items[::-1]
    want = check_case(chroms, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items])
    assert want["seqs"] == [b"ACGTACGTACTTT", (b"NNAGGTTTC" if swap else b"AGGTTTC"), b"AAAA", b"GCA"]


# ------------------------------------------------------------------------------------------------ 7: degenerate calls and errors

def test_no_variants_is_a_copy_and_map_may_be_null():
    chroms = edge_chroms()
    want = check_case(chroms, [], [], [], [])
    assert want["seqs"] == chroms
    g = genome_of(chroms)
    L = _lib.lib()
    h = ctypes.c_void_p()
    ci, ps, rl, ao = np.array([3], dtype=np.int32), np.array([5], dtype=np.int64), np.array([2], dtype=np.int32), np.array([0, 3], dtype=np.int64)
    args = (_lib.ptr(ci, ctypes.c_int32), _lib.ptr(ps, ctypes.c_int64), _lib.ptr(rl, ctypes.c_int32), b"GGN", _lib.ptr(ao, ctypes.c_int64), None, 1, 0)
    assert L.ms_genome_apply_alleles(g.h, *args, ctypes.byref(h), None) == _lib.MS_OK and h.value          # map = NULL
    out = _lib.ResidentGenome.__new__(_lib.ResidentGenome)
    out.h = h
    seqs = chroms[:3] + [chroms[3][:5] + b"GGN" + chroms[3][7:]]
    got, exp = device_planes(out, sum(len(s) for s in seqs)), host_planes(b"".join(seqs))
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    out.close()
    g.close()


def test_invalid_arguments():
    chroms = [b"ACGTACGTAC", b"", b"GGG"]
    g = genome_of(chroms)
    L = _lib.lib()

    def call(chrom, pos, rlen, alts, flags=0, ao=None, alt_null=False, out=True, genome=g.h):
        ci, ps, rl = np.array(chrom, dtype=np.int32), np.array(pos, dtype=np.int64), np.array(rlen, dtype=np.int32)
        ab, off = _lib._flatten_alleles(alts)
        off = off if ao is None else np.array(ao, dtype=np.int64)
        h, hm = ctypes.c_void_p(), ctypes.c_void_p()
        rc = L.ms_genome_apply_alleles(genome, _lib.ptr(ci, ctypes.c_int32), _lib.ptr(ps, ctypes.c_int64), _lib.ptr(rl, ctypes.c_int32),
                                       None if alt_null else ab.tobytes() + b"\0", _lib.ptr(off, ctypes.c_int64), None, len(chrom), flags,
                                       ctypes.byref(h) if out else None, ctypes.byref(hm))
        assert not h.value and not hm.value or rc == _lib.MS_OK
        if rc == _lib.MS_OK:
            L.ms_genome_free(h)
            L.ms_liftmap_free(hm)
        return rc

    INV = _lib.MS_ERR_INVALID
    assert call([0], [3], [1], ["A"]) == _lib.MS_OK
    assert call([3], [0], [1], ["A"]) == INV and call([-1], [0], [1], ["A"]) == INV           # chromosome index
    assert call([0], [11], [0], ["A"]) == INV and call([0], [-1], [1], ["A"]) == INV          # x outside [0, L]
    assert call([0], [10], [0], ["A"]) == _lib.MS_OK                                          # x = L is an insertion point
    assert call([0], [8], [3], ["A"]) == INV and call([0], [2], [-1], ["A"]) == INV           # x + r > L, r < 0
    assert call([1], [0], [0], [""]) == INV                                                   # both alleles empty
    assert call([0], [2], [1], ["A"], ao=[1, 2]) == INV and call([0, 0], [2, 4], [1, 1], ["AA", ""], ao=[0, 2, 1]) == INV
    assert call([0], [2], [1], ["A" * (65536 + 1)]) == INV                                    # MS_ALLELE_MAX_LEN
    assert call([0], [2], [1], ["A"], alt_null=True) == INV
    assert call([0], [2], [1], ["A"], flags=2) == INV and call([0], [2], [1], ["A"], flags=3) == INV
    assert call([0], [2], [1], ["A"], flags=1) == _lib.MS_OK                                  # (the flag without ref_bases changes nothing)
    assert call([0], [2], [1], ["A"], out=False) == INV and call([0], [2], [1], ["A"], genome=None) == INV
    # the lift's own errors
    out, lm = _lib.apply_alleles(g, [0], [2], [1], ["ACG"])
    for lift, lens, other in ((lm.to_alt, [10, 0, 3], [12, 0, 3]), (lm.to_ref, [12, 0, 3], [10, 0, 3])):
        for c, n in enumerate(lens):
            assert lift([c], [n])[0].tolist() == [other[c]]       # the end maps to the end
            with pytest.raises(ValueError):
                lift([c], [n + 1])
        with pytest.raises(ValueError):
            lift([0], [-1])
        with pytest.raises(ValueError):
            lift([3], [0])
        assert lift([], [])[0].size == 0
    assert L.ms_liftmap_lift(lm.h, 2, None, None, 0, None, None) == INV
    # the map outlives both genomes
    out.close()
    g.close()
    assert lm.to_alt([0, 0], [2, 9])[0].tolist() == [2, 11] and lm.to_ref([0], [4])[0].tolist() == [3]
    assert lm.device_ms() > 0 and set(lm.stage_ms()) == {"prep", "order", "host", "splice"}
    lm.close()


# ------------------------------------------------------------------------------------------------ 9: against the existing per-variant splice

SPACED_SEED, SPACED_CUTOFF, SPACED_WIDTHS = 11, 0.1, (6, 9, 12)


def spaced_case():
    """Variants of every kind, further apart than the widest motif plus the longest allele, on three chromosomes (one empty, one short)"""
    rng = np.random.default_rng(SPACED_SEED)
    chroms = [pc.random_dna(rng, 300, 0.01), b"", pc.random_dna(rng, 25, 0.0), pc.random_dna(rng, 260, 0.01)]
    chrom, pos, ref, alt, kind = [], [], [], [], []
    for c in (0, 3, 2):
        x, k = 14, c
        while x + 8 < len(chroms[c]) - 1:
            r = [1, 0, int(rng.integers(1, 9)), int(rng.integers(2, 9))][k % 4]
            a = [1, int(rng.integers(1, 9)), 0, int(rng.integers(2, 9))][k % 4]
            chrom.append(c)
            pos.append(x)
            ref.append(chroms[c][x:x + r].decode())
            alt.append(pc.random_dna(rng, a, 0.0).decode())
            kind.append(k % 4)
            x += 12 + 8 + 12
            k += 1
    return chroms, chrom, pos, ref, alt, np.array(kind)


def test_hits_against_scan_alleles_and_the_reference_genome():
    chroms, chrom, pos, ref, alt, kind = spaced_case()
    V = len(pos)
    mats = [seeded_matrix(w, 40 + w) for w in SPACED_WIDTHS]
    pw = _lib.PwmSet.from_matrices(mats, [SPACED_CUTOFF] * len(mats))
    g = genome_of(chroms)
    rlen, alen = np.array([len(r) for r in ref]), np.array([len(a) for a in alt])
    out, lm = _lib.apply_alleles(g, chrom, pos, rlen, alt, refs=ref)
    assert lm.n_applied == V and not lm.ref_mismatch.any()
    whole = lambda gen: gen.extract(np.arange(len(chroms)), np.zeros(len(chroms), dtype=np.int64), [gen.chrom_sizes[n] for n in gen.names])
    sq_p, sq_r = whole(out), whole(g)
    res_p, res_r = _lib.scan(pw, sq_p, 3), _lib.scan(pw, sq_r, 3)
    hp, hr = res_p.hits(), res_r.hits()
    al = _lib.scan_alleles(pw, g, chrom, pos, rlen, alt)
    rec = al.sites()
    # the shift of the earlier applied variants of the chromosome, per variant
    chrom_a, pos_a = np.array(chrom), np.array(pos)
    shift = np.array([int((alen - rlen)[(chrom_a == chrom_a[v]) & (pos_a < pos_a[v])].sum()) for v in range(V)])
    bits = lambda s: np.asarray(s, dtype=np.float64).view(np.int64)
    n_alt = np.zeros(4, dtype=np.int64)
    n_other = 0
    for m, W in enumerate(SPACED_WIDTHS):
        sel = slice(int(hp["motif_offsets"][m]), int(hp["motif_offsets"][m + 1]))
        p_c, p_q, p_s, p_b = hp["seq_idx"][sel], hp["pos"][sel], hp["strand"][sel].astype(np.int64), bits(hp["score"][sel])
        owner = np.full(p_q.size, -1)
        for v in range(V):                                       # the alt windows of v in the personal genome's coordinates
            lo, hi = pos[v] + shift[v] - W + 1, pos[v] + shift[v] + alen[v] - 1
            owner[(p_c == chrom[v]) & (p_q >= lo) & (p_q <= hi)] = v
        rs = slice(int(rec["motif_offsets"][m]), int(rec["motif_offsets"][m + 1]))
        is_alt = rec["allele"][rs] == 1
        r_v, r_t, r_s, r_b = rec["variant"][rs][is_alt], rec["start"][rs][is_alt], rec["strand"][rs][is_alt].astype(np.int64), bits(rec["score"][rs][is_alt])
        want = sorted(zip(r_v.tolist(), (r_t + shift[r_v]).tolist(), r_s.tolist(), r_b.tolist()))
        inside = owner >= 0
        got = sorted(zip(owner[inside].tolist(), p_q[inside].tolist(), p_s[inside].tolist(), p_b[inside].tolist()))
        assert got == want, m
        np.add.at(n_alt, kind[r_v], 1)
        # every other hit is the reference genome's hit at to_ref(start), and the reference's hits outside every variant's windows are all there
        back, ins = lm.to_ref(p_c[~inside].astype(np.int32), p_q[~inside])
        assert not ins.any()
        got = sorted(zip(p_c[~inside].tolist(), back.tolist(), p_s[~inside].tolist(), p_b[~inside].tolist()))
        sel = slice(int(hr["motif_offsets"][m]), int(hr["motif_offsets"][m + 1]))
        q_c, q_p, q_s, q_b = hr["seq_idx"][sel], hr["pos"][sel], hr["strand"][sel].astype(np.int64), bits(hr["score"][sel])
        touched = np.zeros(q_p.size, dtype=bool)
        for v in range(V):
            touched |= (q_c == chrom[v]) & (q_p >= pos[v] - W + 1) & (q_p <= pos[v] + rlen[v] - 1)
        want = sorted(zip(q_c[~touched].tolist(), q_p[~touched].tolist(), q_s[~touched].tolist(), q_b[~touched].tolist()))
        assert got == want, m
        n_other += len(got)
    assert np.all(n_alt > 0), n_alt                              # alt records of every kind were compared: substitution, insertion, deletion, replacement
    assert n_other > 0                                           # ... and reference hits outside every variant
    # ms_scan_best on one region for one motif: the first maximum of the personal genome's windows, all of which the all-pass scan reports
    one = _lib.PwmSet.from_matrices([mats[1]], [ALL_PASS])
    reg = out.extract([0], [0], [out.chrom_sizes["c0"]])
    allw, best = _lib.scan(one, reg, 3), _lib.scan_best(one, reg, 3)
    h = allw.hits()
    assert len(h["score"]) == 2 * (out.chrom_sizes["c0"] - SPACED_WIDTHS[1] + 1)
    first = int(np.argmax(h["score"]))                          # (hits are in start order, '+' before '-': argmax keeps the first)
    b_score, b_pos, b_strand = best.sites()
    assert bits(b_score[0, 0]) == bits(h["score"][first]) and b_pos[0, 0] == h["pos"][first] and b_strand[0, 0] == h["strand"][first]
    for x in (allw, best, reg, one, al, res_p, res_r, sq_p, sq_r, out, lm, g, pw):
        x.close()


# ------------------------------------------------------------------------------------------------ 10: the downstream entry points

def test_downstream_entry_points_on_the_personal_genome():
    chroms, chrom, pos, ref, alt = pc.random_case(5)
    want = personal.apply_alleles_host(chroms, chrom, pos, ref, alt, lifts=False)
    g = genome_of(chroms)
    out, lm = _lib.apply_alleles(g, chrom, pos, [len(r) for r in ref], alt)
    plain = genome_of(want["seqs"])                              # ms_genome_create of the restatement's strings
    mats = [seeded_matrix(w, 60 + w) for w in (5, 8, 13)]
    pw = _lib.PwmSet.from_matrices(mats, [0.2] * 3)
    assert np.array_equal(out.base_counts(), plain.base_counts())
    rng = np.random.default_rng(2)
    ci = rng.integers(0, len(chroms), 40)
    sizes = want["sizes"][ci]
    st = (rng.random(40) * sizes).astype(np.int64)
    en = np.minimum(st + rng.integers(0, 90, 40), sizes)
    a, b = _lib.scan_regions_once(pw, out, ci, st, en, 3), _lib.scan_regions_once(pw, plain, ci, st, en, 3)
    ha, hb = a.hits(), b.hits()
    assert len(ha["score"]) > 50
    for k in ("motif_offsets", "seq_idx", "pos", "strand"):
        assert np.array_equal(ha[k], hb[k]), k
    assert np.array_equal(ha["score"].view(np.int64), hb["score"].view(np.int64))
    big = int(np.argmax(want["sizes"]))
    s1, s2 = _lib.scan_sweep(pw, out, big, 0, int(want["sizes"][big]), 40, 15, 3), _lib.scan_sweep(pw, plain, big, 0, int(want["sizes"][big]), 40, 15, 3)
    ha, hb = s1.hits(), s2.hits()
    assert len(ha["score"]) > 20
    for k in ("motif_offsets", "seq_idx", "pos", "strand"):
        assert np.array_equal(ha[k], hb[k]), k
    assert np.array_equal(ha["score"].view(np.int64), hb["score"].view(np.int64))
    for x in (a, b, s1, s2, pw, out, lm, plain, g):
        x.close()


# ------------------------------------------------------------------------------------------------ 11: seeded fuzz

@pytest.mark.parametrize("seed", range(40))
def test_seeded_random_cases(seed):
    chroms, chrom, pos, ref, alt = pc.random_case(seed)
    mode = seed % 3                                              # no REF strings / compared and applied / compared and skipped
    want = check_case(chroms, chrom, pos, ref, alt, check=None if mode == 0 else ref, skip=mode == 2)
    if mode == 0:
        assert not want["ref_mismatch"].any()


# ------------------------------------------------------------------------------------------------ 12: Python, end to end

def test_personal_genome_with_a_haplotype_mask_and_scanner():
    rng = np.random.default_rng(13)
    seqs = {"chrA": pc.random_dna(rng, 700, 0.01), "chrB": pc.random_dna(rng, 1200, 0.01)}
    names = list(seqs)
    chrom, pos, ref, alt = [], [], [], []
    for i in range(60):
        c = names[i % 2]
        x = 10 + 18 * (i // 2) + int(rng.integers(0, 6))
        r, a = [(1, 1), (0, 3), (4, 0), (2, 5)][i % 4]
        chrom.append(c); pos.append(x); ref.append(seqs[c][x:x + r].decode()); alt.append(pc.random_dna(rng, a, 0.0).decode())
    select = rng.random(60) < 0.6
    g = _lib.ResidentGenome(seqs)
    out, lm = personal.personal_genome(g, chrom, pos, ref, alt, select=select)
    sel = np.flatnonzero(select)
    assert np.array_equal(lm.selected, sel) and isinstance(out, _lib.ResidentGenome)
    want = personal.apply_alleles_host(seqs, [names.index(chrom[i]) for i in sel], [pos[i] for i in sel], [ref[i] for i in sel], [alt[i] for i in sel])
    assert np.array_equal(lm.status, want["status"]) and lm.n_applied > 20
    spliced = dict(zip(names, want["seqs"]))
    assert out.chrom_sizes == {n: len(s) for n, s in spliced.items()}
    assert out.fetch_sequence("chrB", 5, 400).upper() == spliced["chrB"][5:400].decode().upper()          # through ms_genome_packed_host
    with pytest.raises(ValueError, match="REF is not the genome"):
        personal.personal_genome(g, chrom, pos, [("T" if r[0] in "Aa" else "A") + r[1:] if r else r for r in ref], alt)
    skipped, lm2 = personal.personal_genome(g, chrom[:4], pos[:4], ["T" if ref[0] == "A" else "A"] + ref[1:4], alt[:4], on_mismatch="skip")
    assert lm2.status.tolist()[0] == 2 and lm2.ref_mismatch.tolist() == [1, 0, 0, 0]
    skipped.close()
    lm2.close()

    class Region:
        def __init__(self, c, s, e):
            self.chrom, self.start, self.end, self.summit = c, s, e, (s + e) // 2

    class Pwm:
        def __init__(self, m, c):
            self.matrix, self.cutoffs, self.length = m, {"1e-3": c}, m.shape[1]

    regions = [Region(n, s, min(s + 120, len(spliced[n]))) for n in names for s in range(0, len(spliced[n]) - 20, 90)]
    pwms = [Pwm(seeded_matrix(w, 80 + w), 0.25) for w in (6, 10)]
    plain = _lib.ResidentGenome(spliced)
    a, b = scanner.Scanner(out, regions, 0, "both", "1e-3", remove_dup=False), scanner.Scanner(plain, regions, 0, "both", "1e-3", remove_dup=False)
    got, exp = a.scan_motifs_arrays(pwms, with_tables=True), b.scan_motifs_arrays(pwms, with_tables=True)
    assert len(exp["score"]) > 100
    for k in ("motif", "region", "start", "strand", "motif_offsets", "n_sites"):
        assert np.array_equal(got[k], exp[k]), k
    assert np.array_equal(np.asarray(got["score"]).view(np.int64), np.asarray(exp["score"]).view(np.int64))
    # hits of the personal genome in reference coordinates (Scanner's starts are chromosome positions already: region start 0)
    reg_chrom = np.array([names.index(r.chrom) for r in regions])
    ref_pos, inside = personal.lift_sites(lm, reg_chrom[got["region"]], 0, got["start"])
    exp_pos = np.array([want["to_ref"][c][0][q] for c, q in zip(reg_chrom[got["region"]], got["start"])])
    assert np.array_equal(ref_pos, exp_pos) and inside.sum() > 0
    for x in (a, b, plain, out, lm, g):
        x.close()
