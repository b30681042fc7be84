"""Shuffled control sequences: the sequential restatement of ms_seqset_shuffle (include/motifscan_amd.h, csrc/ms_shuffle.hip).

The device result is specified as a function of (sequence, kind, seed, sequence index) and this module implements that text literally,
one run at a time, with numpy and Python integers only -- no GPU, no library.  The GPU tests compare the device output with it byte for
byte; tests/test_shuffle_host.py pins it to vectors and to the properties a shuffle must have.

  mix(x): x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31          (unsigned 64-bit)
  h(seed, r, x, y) = mix(mix(mix(mix(seed + 0x9e3779b97f4a7c15) + r) + x) + y)

A sequence is cut into its maximal runs of ACGT; every other character stays where it is.  With b the run's start and p a position, both
relative to the sequence's first base, and r the sequence's index in the unsharded set:

  mono   the run's bases ordered by the key (h(seed, r, b, p), p);
  dinuc  Altschul-Erickson: an arborescence towards the run's last base f drawn by Wilson's loop-erased walk (draw d is
         (h(seed, r, b, 2^62 | d) * tot) >> 64 over the off-diagonal counts of the current base), the edge that realises next[u] with the
         largest p is reserved as the last exit of u, every other edge list is ordered by (h(seed, r, b, p), p), and the Euler walk from the
         run's first base reads the lists off.  Runs of fewer than 3 bases are copied.
"""
import numpy as np

KINDS = {"mono": 1, "dinuc": 2}

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_DRAW = 1 << 62
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
_LETTER = "ACGT"


def _mix(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def hash64(seed, r, x, y):
    """h(seed, r, x, y) of the module text; every argument is taken modulo 2^64."""
    v = _mix(((seed & _M64) + _GOLDEN) & _M64)
    v = _mix((v + (r & _M64)) & _M64)
    v = _mix((v + (x & _M64)) & _M64)
    return _mix((v + (y & _M64)) & _M64)


def _prefix(seed, r, b):
    v = _mix(((seed & _M64) + _GOLDEN) & _M64)
    v = _mix((v + (r & _M64)) & _M64)
    return _mix((v + (b & _M64)) & _M64)


def _kind(kind):
    k = KINDS.get(kind, kind)
    if k not in (1, 2):
        raise ValueError("kind must be 'mono' (1) or 'dinuc' (2), not %r" % (kind,))
    return k


def _runs(seq):
    """(start, end) of the maximal ACGT runs of a string"""
    ok = np.frombuffer(seq.encode("latin-1"), dtype=np.uint8)
    ok = np.isin(ok, np.frombuffer(b"ACGTacgt", dtype=np.uint8))
    edge = np.flatnonzero(np.diff(np.concatenate(([0], ok.view(np.int8), [0]))))
    return [(int(edge[i]), int(edge[i + 1])) for i in range(0, edge.size, 2)]


def _mono_run(s, pre, b):
    n = len(s)
    keys = [(_mix((pre + b + i) & _M64), i) for i in range(n)]
    keys.sort()
    return [s[i] for _, i in keys]


def _dinuc_run(s, pre, b):
    n = len(s)
    if n < 3:
        return list(s)
    m = [[0] * 4 for _ in range(4)]
    for i in range(n - 1):
        m[s[i]][s[i + 1]] += 1
    f = s[n - 1]
    in_tree = [False] * 4
    in_tree[f] = True
    nxt = [-1] * 4
    d = 0
    for v in range(4):
        if in_tree[v] or not any(m[v]):
            continue
        u = v
        while not in_tree[u]:
            tot = sum(m[u][w] for w in range(4) if w != u)
            x = (_mix((pre + (_DRAW | d)) & _M64) * tot) >> 64
            d += 1
            acc = 0
            for w in range(4):
                if w == u:
                    continue
                acc += m[u][w]
                if acc > x:
                    break
            nxt[u] = w
            u = w
        u = v
        while not in_tree[u]:
            in_tree[u] = True
            u = nxt[u]
    reserved = [-1] * 4
    for i in range(n - 1):
        u = s[i]
        if u != f and s[i + 1] == nxt[u]:
            reserved[u] = i
    order = sorted(range(n - 1), key=lambda i: (s[i], 1 if reserved[s[i]] == i else 0, _mix((pre + b + i) & _M64), i))
    lists = [[], [], [], []]
    for i in order:
        lists[s[i]].append(s[i + 1])
    ptr = [0] * 4
    out = [s[0]]
    cur = s[0]
    for _ in range(n - 1):
        k = ptr[cur]
        ptr[cur] = k + 1
        cur = lists[cur][k]
        out.append(cur)
    assert cur == f and all(ptr[u] == len(lists[u]) for u in range(4))
    return out


def shuffle_host(seqs, kind, seed, seq_index_base=0):
    """The shuffled sequences as a list of str: sequence k is shuffled as sequence seq_index_base + k.  Non-ACGT characters are kept as
    they are, ACGT come out in upper case."""
    k = _kind(kind)
    if seq_index_base < 0:
        raise ValueError("seq_index_base must be >= 0")
    out = []
    for j, seq in enumerate(seqs):
        chars = list(seq)
        for b, e in _runs(seq):
            s = [_CODE[ch] for ch in seq[b:e]]
            pre = _prefix(seed, seq_index_base + j, b)
            res = _mono_run(s, pre, b) if k == 1 else _dinuc_run(s, pre, b)
            chars[b:e] = [_LETTER[c] for c in res]
        out.append("".join(chars))
    return out


def dinuc_counts(seq):
    """The 16 dinucleotide counts [first base][second base] of every ACGT run of a string, in order: a list of (4, 4) int64 arrays.  A pair
    that spans a non-ACGT character belongs to no run and is not counted."""
    res = []
    for b, e in _runs(seq):
        m = np.zeros((4, 4), dtype=np.int64)
        for i in range(b, e - 1):
            m[_CODE[seq[i]], _CODE[seq[i + 1]]] += 1
        res.append(m)
    return res
