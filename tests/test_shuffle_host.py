"""
CPU-only: motifscan_amd/shuffle.py, the sequential restatement of ms_seqset_shuffle (include/motifscan_amd.h), pinned to the
specification's vectors and to the properties a mono- / dinucleotide shuffle must have -- what the device output is then compared with
byte for byte (tests/test_gpu_shuffle.py).  No GPU, no library call except the symbol checks at the end.
"""
import ctypes
import itertools

import numpy as np
import pytest

import shuffle_cases as sc
from motifscan_amd import shuffle


def test_hash_vectors():
    for args, want in sc.HASH_VECTORS:
        assert shuffle.hash64(*args) == want, args
    assert shuffle.KINDS == {"mono": 1, "dinuc": 2}


def test_end_to_end_vectors():
    for kind, seed, r, want in sc.VECTORS:
        got = shuffle.shuffle_host([sc.VECTOR_IN], kind, seed, seq_index_base=r)
        assert got == [want], (kind, seed, r)
        assert shuffle.shuffle_host([sc.VECTOR_IN], shuffle.KINDS[kind], seed, r) == [want]


@pytest.mark.parametrize("kind", ["mono", "dinuc"])
def test_properties_on_random_sequences(kind):
    rng = np.random.default_rng(20240917)
    lengths = list(range(0, 301, 3)) + rng.integers(0, 301, size=99).tolist()
    assert len(lengths) == 200 and min(lengths) == 0 and max(lengths) == 300
    seqs = []
    for i, n in enumerate(lengths):
        seqs.append(sc.random_sequence(rng, int(n), letters=1 + i % 4, dirt=(0.0, 0.02, 0.15, 0.4)[(i // 4) % 4]))
    assert any(set(s) - set("ACGT") for s in seqs) and any(s.isupper() and not set(s) - set("ACGT") for s in seqs)
    out = shuffle.shuffle_host(seqs, kind, seed=11)
    assert len(out) == len(seqs)
    changed = 0
    for s, o in zip(seqs, out):
        sc.check_properties(s, o, kind)
        changed += s.upper() != o.upper()
    assert changed > 100


@pytest.mark.parametrize("kind", ["mono", "dinuc"])
def test_short_and_low_complexity_runs(kind):
    out = shuffle.shuffle_host(sc.HAND_SET, kind, seed=3)
    for s, o in zip(sc.HAND_SET, out):
        sc.check_properties(s, o, kind)
    by_in = dict(zip(sc.HAND_SET, out))
    for s in ("", "A", "N", "TTTTTTTTTTTTTTTTTTTT"):
        assert by_in[s] == s
    if kind == "dinuc":
        for s in ("AC", "ACG", "A" * 200 + "C", "AC" * 100 + "G"):          # fewer than 3 bases, or only one Euler path
            assert by_in[s] == s
        assert by_in["NANCANACGN"] == "NANCANACGN"
    else:
        assert sorted(by_in["A" * 200 + "C"]) == ["A"] * 200 + ["C"] and by_in["A" * 200 + "C"] != "A" * 200 + "C"


def test_deterministic_and_sensitive_to_seed_and_index():
    rng = np.random.default_rng(5)
    s = sc.random_sequence(rng, 60, 4, 0.0)
    for kind in ("mono", "dinuc"):
        a = shuffle.shuffle_host([s], kind, 1)
        assert a == shuffle.shuffle_host([s], kind, 1)
        assert a != shuffle.shuffle_host([s], kind, 2)
        assert a != shuffle.shuffle_host([s], kind, 1, seq_index_base=1)
        assert a != [s]
        assert shuffle.shuffle_host([s, s], kind, 1)[1] == shuffle.shuffle_host([s], kind, 1, seq_index_base=1)[0]


def test_seq_index_base_is_the_tail_of_the_whole():
    rng = np.random.default_rng(6)
    seqs = [sc.random_sequence(rng, int(n), 4, 0.05) for n in rng.integers(0, 80, size=12)]
    for kind in ("mono", "dinuc"):
        whole = shuffle.shuffle_host(seqs, kind, 9)
        for k in (0, 1, 5, 11, 12):
            assert shuffle.shuffle_host(seqs[k:], kind, 9, seq_index_base=k) == whole[k:]


def test_argument_checks():
    with pytest.raises(ValueError):
        shuffle.shuffle_host(["ACGT"], "trinuc", 0)
    with pytest.raises(ValueError):
        shuffle.shuffle_host(["ACGT"], 3, 0)
    with pytest.raises(ValueError):
        shuffle.shuffle_host(["ACGT"], "mono", 0, seq_index_base=-1)
    assert shuffle.shuffle_host([], "dinuc", 0) == []


def test_dinuc_counts_respect_run_boundaries():
    got = shuffle.dinuc_counts("ACNGT")
    assert len(got) == 2 and got[0][0, 1] == 1 and got[0].sum() == 1 and got[1][2, 3] == 1 and got[1].sum() == 1
    assert shuffle.dinuc_counts("NN") == [] and shuffle.dinuc_counts("") == []
    one = shuffle.dinuc_counts("a")
    assert len(one) == 1 and one[0].sum() == 0
    assert shuffle.dinuc_counts("acgt")[0].sum() == 3


def euler_sequences(s):
    """every sequence with the dinucleotide counts, first and last base of s: a DFS over the Euler paths of its edge multigraph"""
    m = {}
    for a, b in zip(s, s[1:]):
        m[(a, b)] = m.get((a, b), 0) + 1
    found = set()

    def walk(path, left):
        if left == 0:
            found.add("".join(path))
            return
        u = path[-1]
        for w in "ACGT":
            if m.get((u, w), 0) > 0:
                m[(u, w)] -= 1
                path.append(w)
                walk(path, left - 1)
                path.pop()
                m[(u, w)] += 1

    walk([s[0]], len(s) - 1)
    return found


def chi_square(counts, n_total, n_cells):
    e = n_total / n_cells
    return float(sum((c - e) ** 2 / e for c in counts))


def test_dinuc_is_uniform_over_the_euler_paths():
    s = "ACAGCCAGGCAAT"
    want = euler_sequences(s)
    assert len(want) == 72 and s in want
    seen = {}
    for seed in range(14400):
        o = shuffle.shuffle_host([s], "dinuc", seed)[0]
        seen[o] = seen.get(o, 0) + 1
    assert set(seen) == want
    chi2 = chi_square(seen.values(), 14400, 72)
    print("dinuc chi2 over 72 cells:", chi2)
    assert chi2 < 125.0                      # the 1e-4 tail at 71 degrees of freedom; the run is deterministic


def test_mono_is_uniform_over_the_arrangements():
    s = "AACGT"
    want = {"".join(p) for p in itertools.permutations(s)}
    assert len(want) == 60
    seen = {}
    for seed in range(6000):
        o = shuffle.shuffle_host([s], "mono", seed)[0]
        seen[o] = seen.get(o, 0) + 1
    assert set(seen) == want
    chi2 = chi_square(seen.values(), 6000, 60)
    print("mono chi2 over 60 cells:", chi2)
    assert chi2 < 110.0                      # the 1e-4 tail at 59 degrees of freedom


def test_library_declares_and_exports_the_shuffle_entry_points():
    import os
    import re
    from motifscan_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "motifscan_amd.h")).read()
    assert re.search(r"\bint\s+ms_seqset_shuffle\s*\(", text) and re.search(r"\bint\s+ms_seqset_packed_host\s*\(", text)
    assert re.search(r"#define\s+MS_SHUFFLE_MONO\s+1\b", text) and re.search(r"#define\s+MS_SHUFFLE_DINUC\s+2\b", text)
    L = _lib.lib()
    dims = _lib.shuffle_dims()                                   # needs no GPU
    assert 3 <= dims["lane_run"] <= dims["lds_run"] and dims["block_bases"] % 32 == 0 and dims["reserved"] == 0
    assert L.ms_debug_shuffle_dims(None) == _lib.MS_ERR_INVALID
    assert L.ms_debug_shuffle_stage_ms(None) == _lib.MS_ERR_INVALID
    out = ctypes.c_void_p()
    assert L.ms_seqset_shuffle(None, 2, 0, 0, 0, None) == _lib.MS_ERR_INVALID          # NULL out: before any device is looked for
    assert L.ms_seqset_packed_host(None, None, None) == _lib.MS_ERR_INVALID
    if _lib.device_count() == 0:
        assert L.ms_seqset_shuffle(None, 2, 0, 0, 0, ctypes.byref(out)) == _lib.MS_ERR_RUNTIME     # no CPU fallback
