"""Pairwise sequence alignment of many pairs, clustering by sequence identity and matching two structures by alignment, on the GPU
(Needleman and Wunsch 1970; Smith and Waterman 1981; Gotoh 1982, the affine gap in three states).

Every other module matches two structures by chain name and residue number (lddt.match_atoms); tmscore.py and lddt.py say under "Not built"
that no alignment search exists, and that stays true of THEM: they are for a given correspondence. This module makes one from the sequences
(6I9F.pdb numbers its residues -11 .. 143, the package's own output of it 1 .. 155), and it gives the training pipeline what lay between
pesto_amd.dataset and pesto_amd.training: clusters of subunits by sequence identity, and the split of a dataset by cluster (the reference's
processing/split_dataset.ipynb downloads RCSB's clusters at 30 % identity for that). All on pesto_align.hip:
    align_scores          AlignScores(score, n_ident, n_aligned, n_cols, span) of listed pairs, or of all i < j
    align_maps            AlignMaps: the same plus map / map_offsets, the alignment itself, for a short list
    identity              n_ident over a chosen length, float64, for reading only
    cluster_sequences     labels int32 [S]: single linkage over the pairs that pass integer thresholds, linked in the scoring launch
    split_clusters        (train, test, validation) index arrays by cluster (host only)
    structure_sequences   per protein chain (chain_name, codes, first atom of each residue)
    match_atoms           lddt.match_atoms' five results with the residues matched by alignment; structure_lddt, structure_tmscore over it
    encode, match_matrix, BLOSUM62, AMINO
The lead argument decides where a call runs (_lib.Side): host arrays in, NumPy out; (codes, offsets) with codes a ROCm tensor in, ROCm
tensors out on torch's current stream. ``model`` lends its device handle. There is no CPU or PyTorch fallback. Arguments are checked on
the host before any launch (ValueError); the codes are checked again by a kernel whose verdict is read before anything is written
(PestoError). Every output is an integer, bit-identical from call to call, between host and device inputs, and between a pair scored
alone and in a batch.

Definition.
Sequences. A sequence is a uint8 array of codes in [0, A). The default alphabet is AMINO = "ARNDCQEGHILKMFPSTWYV" plus X = 20, so A = 21;
encode(str) maps every other letter to X. 1 <= length <= MAX_LENGTH = 4096 and A <= 32.
Matrix and gaps. matrix is int8 [A, A] (s(x, y) = matrix[x, y]; it need not be symmetric). A gap of k residues costs go + (k - 1) ge with
integers 127 >= go = gap_open >= ge = gap_extend >= 0 (defaults 11 and 1). unknown= names a code that never counts as identical (default
20, None: no such code).
Three states per cell (i, j), 0 <= i <= m, 0 <= j <= n, for a of m codes against b of n:
    D[i][j] = s(a[i-1], b[j-1]) + max(D, U, L)[i-1][j-1]                        aligns a[i-1] to b[j-1]
    U[i][j] = max(D[i-1][j] - go, U[i-1][j] - ge, L[i-1][j] - go)               sets a[i-1] against a gap
    L[i][j] = max(D[i][j-1] - go, U[i][j-1] - go, L[i][j-1] - ge)               sets b[j-1] against a gap
Where several candidates are equal, THE FIRST IN THE ORDER D, U, L IS THE PREDECESSOR. Minus infinity is a sentinel that can neither
overflow nor win; every sum fits int32 (|score| <= 127 * 8192).
Modes.
    "global"   D[0][0] = 0, U[i][0] = -(go + (i - 1) ge), L[0][j] likewise, everything else on the border minus infinity. The end is at
               (m, n), in the best of D, U, L, ties in that order.
    "overlap"  end gaps free in both sequences: D[i][0] = D[0][j] = 0 are start cells, U and L on the border minus infinity. The end is
               the maximum of D over the cells with i = m or j = n (the start cells (m, 0) and (0, n) among them), ties to the smallest
               i, then the smallest j. So when no other such cell is positive the end is (0, n): score 0, no column, span (0, n, 0, n).
    "local"    the border is minus infinity and D may start fresh: D[i][j] = s + max(D, U, L, 0), the fresh start being the LAST candidate.
               The end is the maximum of D over all cells with i, j >= 1, the same tie rule. If no D is positive the alignment is empty:
               score 0, counts 0, span (0, 0, 0, 0).
Canonical alignment: the path from the end back through the predecessors just defined. There is exactly one.
Outputs per pair, all int32: score; n_ident, the D columns with equal codes that are not ``unknown``; n_aligned, the D columns; n_cols,
all columns; span = (i0, j0, i1, j1), the half-open ranges of a and of b that the path covers. align_scores stores no cell matrix and
walks nothing back: every state carries n_ident, n_aligned, i0 and j0 of its own path through the same choice that picks its value
(n_cols = (i1 - i0) + (j1 - j0) - n_aligned); a pair costs O(m + n) memory.
Map. align_maps returns map int32, ragged over a's residues (pair p owns map[map_offsets[p]:map_offsets[p + 1]], m entries): the index in
b that a[i] is aligned to, -1 where a[i] faces a gap or lies outside the span. It stores one byte per cell and walks the path back on
the device; its list is run in chunks of at most 256 MiB of such bytes (a 4096 x 4096 pair needs 16 MiB). Its five other outputs are
counted on that walk and equal align_scores' to the bit.
Clusters. A pair links its two sequences when
    n_ident * 10000 >= id_bp * denom   and   n_aligned * 10000 >= cov_bp * max(m, n)   and   denom > 0
in 64-bit integers, id_bp = round(min_identity * 10000) and cov_bp likewise, rounded once on the host; denom by over=: "shorter" = min(m, n)
(the default), "aligned" = n_aligned, "columns" = n_cols. No float decides a link. labels numbers the connected components (single linkage:
A-B and B-C put A and C together whether or not A-C passes) in the order of their smallest members. The links are made by the waves that
score the pairs; no S x S matrix exists. cluster_sequences makes two exact reductions before the launch. Byte-identical sequences are
collapsed onto their first copy: every pair among a sequence o and its copies is the pair (o, o), and a copy has o's links to everything
else, so the copies join o's component if (o, o) passes (one more align_scores call, over the duplicated sequences only, and the same
integer test on the host) or if o has any link, and otherwise stay alone, as o does. With min_coverage > 0 the pairs with
min(m, n) * 10000 < cov_bp * max(m, n) are not enumerated, because n_aligned <= min(m, n).
Neither changes labels. There is no k-mer or other inexact prefilter.

Not built (structure-based alignment is structalign.py's): profile or multiple alignment, k-mer prefilters and database-scale search, nucleic
acids, sequences above 4096, packed 16-bit arithmetic. (Chain permutation beyond the greedy pairing of match_atoms: chainmap.py.)

Limits: 1 <= length <= MAX_LENGTH, A <= 32, gap_open <= 127, S <= 2**20, at most 2**31 - 1 pairs per call (2**20 for align_maps).
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .trajectory import _model_of

MAX_LENGTH = 4096               # PESTO_ALIGN_MAX_LENGTH
MAX_ALPHABET = 32               # PESTO_ALIGN_MAX_ALPHABET
MAX_GAP = 127                   # PESTO_ALIGN_MAX_GAP
MAX_SEQUENCES = 2 ** 20         # PESTO_ALIGN_MAX_SEQUENCES
MAX_PAIRS = 2 ** 31 - 1         # PESTO_ALIGN_MAX_PAIRS
MAX_MAP_PAIRS = 2 ** 20         # PESTO_ALIGN_MAX_MAP_PAIRS
MAPS_WORKSPACE = 2 ** 28        # PESTO_ALIGN_MAPS_WORKSPACE
AMINO = "ARNDCQEGHILKMFPSTWYV"
UNKNOWN = 20                    # X
MODES = {"global": 0, "overlap": 1, "local": 2}
OVER = {"shorter": 0, "aligned": 1, "columns": 2}
THREE_TO_ONE = dict(ALA="A", ARG="R", ASN="N", ASP="D", CYS="C", GLN="Q", GLU="E", GLY="G", HIS="H", ILE="I", LEU="L", LYS="K", MET="M",
                    PHE="F", PRO="P", SER="S", THR="T", TRP="W", TYR="Y", VAL="V")

AlignScores = namedtuple("AlignScores", "score n_ident n_aligned n_cols span")
AlignMaps = namedtuple("AlignMaps", "score n_ident n_aligned n_cols span map map_offsets")

_BLOSUM62_ROWS = """
 4 -1 -2 -2  0 -1 -1  0 -2 -1 -1 -1 -1 -2 -1  1  0 -3 -2  0
-1  5  0 -2 -3  1  0 -2  0 -3 -2  2 -1 -3 -2 -1 -1 -3 -2 -3
-2  0  6  1 -3  0  0  0  1 -3 -3  0 -2 -3 -2  1  0 -4 -2 -3
-2 -2  1  6 -3  0  2 -1 -1 -3 -4 -1 -3 -3 -1  0 -1 -4 -3 -3
 0 -3 -3 -3  9 -3 -4 -3 -3 -1 -1 -3 -1 -2 -3 -1 -1 -2 -2 -1
-1  1  0  0 -3  5  2 -2  0 -3 -2  1  0 -3 -1  0 -1 -2 -1 -2
-1  0  0  2 -4  2  5 -2  0 -3 -3  1 -2 -3 -1  0 -1 -3 -2 -2
 0 -2  0 -1 -3 -2 -2  6 -2 -4 -4 -2 -3 -3 -2  0 -2 -2 -3 -3
-2  0  1 -1 -3  0  0 -2  8 -3 -3 -1 -2 -1 -2 -1 -2 -2  2 -3
-1 -3 -3 -3 -1 -3 -3 -4 -3  4  2 -3  1  0 -3 -2 -1 -3 -1  3
-1 -2 -3 -4 -1 -2 -3 -4 -3  2  4 -2  2  0 -3 -2 -1 -2 -1  1
-1  2  0 -1 -3  1  1 -2 -1 -3 -2  5 -1 -3 -1  0 -1 -3 -2 -2
-1 -1 -2 -3 -1  0 -2 -3 -2  1  2 -1  5  0 -2 -1 -1 -1 -1  1
-2 -3 -3 -3 -2 -3 -3 -3 -1  0  0 -3  0  6 -4 -2 -2  1  3 -1
-1 -2 -2 -1 -3 -1 -1 -2 -2 -3 -3 -1 -2 -4  7 -1 -1 -4 -3 -2
 1 -1  1  0 -1  0  0  0 -1 -2 -2  0 -1 -2 -1  4  1 -3 -2 -2
 0 -1  0 -1 -1 -1 -1 -2 -2 -1 -1 -1 -1 -2 -1  1  5 -2 -2  0
-3 -3 -4 -4 -2 -2 -3 -2 -2 -3 -2 -3 -1  1 -4 -3 -2 11  2 -3
-2 -2 -2 -3 -2 -1 -2 -3  2 -1 -1 -2 -1  3 -3 -2 -2  2  7 -1
 0 -3 -3 -3 -1 -2 -2 -3 -3  3  1 -2  1 -1 -2 -2  0 -3 -1  4
"""


def _blosum62():
    """BLOSUM62 (Henikoff and Henikoff 1992) in the order of AMINO, the X row and column -1. The table was typed in from memory, not
    copied from a file: compare it with the BLOSUM62 file that NCBI BLAST distributes (or Biopython's substitution_matrices) before
    relying on a particular entry. Nothing in the package depends on its values; a test pins its symmetry and its diagonal."""
    m = np.full((21, 21), -1, np.int8)
    m[:20, :20] = np.array(_BLOSUM62_ROWS.split(), np.int8).reshape(20, 20)
    m.setflags(write=False)
    return m


BLOSUM62 = _blosum62()
_CODE_OF = np.full(256, UNKNOWN, np.uint8)
_CODE_OF[np.frombuffer(AMINO.encode(), np.uint8)] = np.arange(20, dtype=np.uint8)


def encode(text):
    """uint8 [len(text)]: the codes of a one-letter protein sequence, AMINO's letters 0 .. 19, every other character X = 20"""
    if isinstance(text, str):
        text = text.encode("latin-1", "replace")
    if not isinstance(text, (bytes, bytearray)):
        raise ValueError(f"encode takes a str or bytes, got {type(text).__name__}")
    return _CODE_OF[np.frombuffer(bytes(text), np.uint8)]


def match_matrix(match=1, mismatch=-1, A=21):
    """int8 [A, A]: ``match`` on the diagonal, ``mismatch`` elsewhere"""
    if any(isinstance(v, bool) or v != int(v) for v in (match, mismatch, A)) or not 1 <= A <= MAX_ALPHABET or not -128 <= match <= 127 or not -128 <= mismatch <= 127:
        raise ValueError(f"int8 scores and 1 <= A <= {MAX_ALPHABET} expected, got {match!r}, {mismatch!r}, {A!r}")
    m = np.full((int(A), int(A)), int(mismatch), np.int8)
    np.fill_diagonal(m, int(match))
    return m


# ------------------------------------------------------------------ arguments
def _sequences(seqs):
    """(codes: uint8 [total] host array or ROCm tensor, offsets int32 [S + 1] on the host) of a seqs argument"""
    if isinstance(seqs, tuple) and len(seqs) == 2 and not isinstance(seqs[0], (str, bytes)):
        codes, offs = seqs
        offs = np.asarray(_lib.host(offs)).reshape(-1)
        if offs.size < 2 or not np.issubdtype(offs.dtype, np.integer) or offs[0] != 0 or np.any(np.diff(offs.astype(np.int64)) < 1):
            raise ValueError("offsets must be integers ascending from 0 over non-empty sequences")
        total = int(offs[-1])
        if total >= 2 ** 31:
            raise ValueError("at most 2**31 - 1 codes per call")
        if _lib.is_torch(codes):
            import torch
            if codes.dtype != torch.uint8 or codes.dim() != 1 or codes.shape[0] != total:
                raise ValueError(f"codes must be uint8 [{total}], got {codes.dtype} {list(codes.shape)}")
        else:
            codes = _codes(codes)
            if codes.size != total:
                raise ValueError(f"codes must be uint8 [{total}], got [{codes.size}]")
        offs = np.ascontiguousarray(offs, np.int32)
    else:
        if isinstance(seqs, (str, bytes)) or not hasattr(seqs, "__len__") or len(seqs) < 1:
            raise ValueError("seqs must be a non-empty list of sequences (strings or code arrays), or (codes, offsets)")
        parts = [encode(s) if isinstance(s, (str, bytes)) else _codes(s) for s in seqs]
        if sum(p.size for p in parts) >= 2 ** 31:
            raise ValueError("at most 2**31 - 1 codes per call")
        offs = _lib.offsets([p.size for p in parts])
        codes = np.concatenate(parts)
    S = offs.size - 1
    L = np.diff(offs)
    if S > MAX_SEQUENCES:
        raise ValueError(f"at most {MAX_SEQUENCES} sequences per call, got {S}")
    if L.min() < 1 or L.max() > MAX_LENGTH:
        s = int(np.argmax((L < 1) | (L > MAX_LENGTH)))
        raise ValueError(f"a sequence has 1 to {MAX_LENGTH} codes, sequence {s} has {int(L[s])}")
    return codes, offs


def _codes(a):
    a = _lib.host(a)
    if a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_):
        raise ValueError(f"a sequence is a string or a one-dimensional array of integer codes, got {a.dtype} {list(a.shape)}")
    if a.size and (a.min() < 0 or a.max() > 255):
        raise ValueError("codes must lie in [0, A)")
    return np.ascontiguousarray(a, np.uint8)


def _scoring(codes, mode, matrix, gap_open, gap_extend, unknown):
    """(mode code, matrix int8 [A, A], A, go, ge, unknown code or -1), checked; host codes are checked against A here"""
    if mode not in MODES:
        raise ValueError(f"mode must be 'global', 'overlap' or 'local', got {mode!r}")
    mat = _lib.host(matrix)
    if mat.ndim != 2 or mat.shape[0] != mat.shape[1] or not 1 <= mat.shape[0] <= MAX_ALPHABET or not np.issubdtype(mat.dtype, np.integer) \
            or mat.min() < -128 or mat.max() > 127:
        raise ValueError(f"matrix must be int8 [A, A] with A <= {MAX_ALPHABET}, got {mat.dtype} {list(mat.shape)}")
    A = int(mat.shape[0])
    for v in (gap_open, gap_extend):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"gap_open and gap_extend must be integers, got {gap_open!r}, {gap_extend!r}")
    if not MAX_GAP >= gap_open >= gap_extend >= 0:
        raise ValueError(f"{MAX_GAP} >= gap_open >= gap_extend >= 0 expected, got {gap_open}, {gap_extend}")
    if unknown is None:
        unknown = -1
    elif isinstance(unknown, bool) or not isinstance(unknown, (int, np.integer)) or not 0 <= unknown < MAX_ALPHABET:
        raise ValueError(f"unknown must be a code or None, got {unknown!r}")
    elif unknown >= A:
        unknown = -1                                # (a code the alphabet does not have never occurs)
    if not _lib.is_torch(codes) and codes.size and int(codes.max()) >= A:
        raise ValueError(f"every code must lie in [0, {A})")
    return MODES[mode], np.ascontiguousarray(mat, np.int8), A, int(gap_open), int(gap_extend), int(unknown)


def _pairs(pairs, S, least=0, most=MAX_PAIRS):
    p = _lib.host(pairs)
    if p.size == 0:
        p = p.reshape(0, 2).astype(np.int32)
    if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"pairs must be integers [P, 2], got {p.dtype} {list(p.shape)}")
    if not least <= p.shape[0] <= most:
        raise ValueError(f"{least} to {most} pairs per call, got {p.shape[0]}")
    if p.size and (p.min() < 0 or p.max() >= S):
        raise ValueError(f"pairs must name sequences 0 .. {S - 1}")
    return np.ascontiguousarray(p, np.int32)


def _call(seqs, pairs, mode, matrix, gap_open, gap_extend, unknown, model, want, thresholds=None):
    """the one route to the two entry points. want: 'scores', 'maps' or 'labels' (thresholds = (id_bp, cov_bp, over code))"""
    codes, offs = _sequences(seqs)
    S = offs.size - 1
    mcode, mat, A, go, ge, unk = _scoring(codes, mode, matrix, gap_open, gap_extend, unknown)
    if pairs is None:
        if want == "maps":
            raise ValueError("align_maps takes an explicit list of pairs")
        P, pl = S * (S - 1) // 2, None
        if P > MAX_PAIRS:
            raise ValueError(f"{P} pairs: at most 2**31 - 1 per call")
    else:
        pl = _pairs(pairs, S, *((1, MAX_MAP_PAIRS) if want == "maps" else ()))
        P = int(pl.shape[0])
    model = _model_of(model, codes)
    side = _lib.Side(codes, model._gpu)
    cd = side.put(codes, np.uint8)
    lib = _lib.load()
    pp = None if pl is None else pl.ctypes.data
    head = (model.handle, S, offs.ctypes.data, side.ptr(cd), A, mat.ctypes.data, mcode, go, ge, unk, P, pp)
    if want == "labels":
        labels = side.empty((S,), np.int32)
        _lib.check(lib.pesto_align_scores(*head, None, None, None, None, None, *thresholds, side.ptr(labels), side.kind, side.stream),
                   lib.pesto_align_last_error)
        return side.result(labels)
    out = [side.empty((P,), np.int32) for _ in range(4)] + [side.empty((P, 4), np.int32)]
    if want == "scores":
        _lib.check(lib.pesto_align_scores(*head, *(side.ptr(v) for v in out), 0, 0, 0, None, side.kind, side.stream), lib.pesto_align_last_error)
        return AlignScores(*(side.result(v) for v in out))
    moff = np.zeros(P + 1, np.int64)
    np.cumsum(np.diff(offs)[pl[:, 0]], out=moff[1:])
    amap = side.empty((int(moff[-1]),), np.int32)
    _lib.check(lib.pesto_align_maps(*head, *(side.ptr(v) for v in out), side.ptr(amap), side.kind, side.stream), lib.pesto_align_last_error)
    return AlignMaps(*(side.result(v) for v in out), side.result(amap), moff)


def align_scores(seqs, pairs=None, *, mode="global", matrix=BLOSUM62, gap_open=11, gap_extend=1, unknown=UNKNOWN, model=None):
    """AlignScores(score, n_ident, n_aligned, n_cols int32 [P], span int32 [P, 4]) of the pairs (a, b) listed in ``pairs`` [P, 2]
    (indices into seqs; host memory), or of all i < j in row-major order. seqs: a list of strings or code arrays, or (codes uint8
    [total], offsets [S + 1]). See the module's definition."""
    return _call(seqs, pairs, mode, matrix, gap_open, gap_extend, unknown, model, "scores")


def align_maps(seqs, pairs, *, mode="global", matrix=BLOSUM62, gap_open=11, gap_extend=1, unknown=UNKNOWN, model=None):
    """AlignMaps: align_scores' five fields, then map int32 [sum of m] and map_offsets int64 [P + 1] (host): pair p's rows give, for every
    residue of its a, the index in b it is aligned to, or -1."""
    return _call(seqs, pairs, mode, matrix, gap_open, gap_extend, unknown, model, "maps")


def identity(result, lengths_a, lengths_b, over="shorter"):
    """float64 [P]: n_ident over min(m, n) ("shorter"), n_aligned ("aligned") or n_cols ("columns"); 0 where that is 0. On the host, for
    reading: decisions (cluster_sequences, match_atoms) never use it."""
    if over not in OVER:
        raise ValueError(f"over must be 'shorter', 'aligned' or 'columns', got {over!r}")
    ni = _lib.host(result.n_ident).astype(np.float64)
    if over == "shorter":
        d = np.minimum(np.asarray(_lib.host(lengths_a), np.float64), np.asarray(_lib.host(lengths_b), np.float64))
    else:
        d = _lib.host(result.n_aligned if over == "aligned" else result.n_cols).astype(np.float64)
    if d.shape != ni.shape:
        raise ValueError(f"lengths must be [{ni.size}], got {list(d.shape)}")
    return np.divide(ni, d, out=np.zeros_like(ni), where=d > 0)


def _basis_points(v, name):
    v = float(v)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"{name} must lie in [0, 1], got {v!r}")
    return int(round(v * 10000))


def cluster_sequences(seqs, min_identity=0.3, min_coverage=0.0, over="shorter", mode="global", *, matrix=BLOSUM62, gap_open=11, gap_extend=1,
                      unknown=UNKNOWN, model=None, _reduce=True):
    """labels int32 [S]: the connected components of the sequences under the module's integer link test, numbered in the order of their
    smallest members. All against all in one launch, the links made by the waves that score. (_reduce=False switches the two exact
    host-side reductions off; the labels are the same.)"""
    if over not in OVER:
        raise ValueError(f"over must be 'shorter', 'aligned' or 'columns', got {over!r}")
    thr = (_basis_points(min_identity, "min_identity"), _basis_points(min_coverage, "min_coverage"), OVER[over])
    codes, offs = _sequences(seqs)
    S = offs.size - 1
    L = np.diff(offs).astype(np.int64)
    if not _reduce:
        return _call((codes, offs), None, mode, matrix, gap_open, gap_extend, unknown, model, "labels", thr)
    # byte-identical sequences onto their first copy
    hc = _lib.host(codes)
    first, rep = {}, np.zeros(S, np.int64)
    for s in range(S):
        rep[s] = first.setdefault(hc[offs[s]:offs[s + 1]].tobytes(), s)
    keep = np.nonzero(rep == np.arange(S))[0]
    sub = (codes, offs)
    if keep.size < S:
        sub = (np.concatenate([hc[offs[s]:offs[s + 1]] for s in keep]), _lib.offsets(L[keep]))
        if _lib.is_torch(codes) and codes.is_cuda:
            import torch
            sub = (torch.from_numpy(sub[0]).to(codes.device), sub[1])
    pairs = None
    if thr[1] > 0:
        # only the pairs that the lengths leave possible: n_aligned <= min(m, n), so min(m, n) * 10000 >= cov_bp * max(m, n) is necessary
        Lk = L[keep]
        order = np.argsort(Lk, kind="stable")
        Ls = Lk[order]
        rows = []
        for x in range(order.size):
            hi = int(np.searchsorted(Ls, (Ls[x] * 10000) // thr[1], "right"))       # partners y > x: Ls[y] >= Ls[x]
            if hi > x + 1:
                y = order[x + 1:hi]
                rows.append(np.stack([np.minimum(order[x], y), np.maximum(order[x], y)], 1))
        pairs = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 2), np.int32)
        if pairs.shape[0] > MAX_PAIRS:
            raise ValueError(f"{pairs.shape[0]} pairs: at most 2**31 - 1 per call")
    labels = _call(sub, pairs, mode, matrix, gap_open, gap_extend, unknown, model, "labels", thr)
    if keep.size == S:
        return labels
    # The copies of a sequence o. Every pair among o and its copies is the pair (o, o), and a copy has o's links to everything else. So
    # they join o's component if (o, o) passes or o has any link; otherwise each stays alone, as o does.
    kl = np.asarray(_lib.host(labels)).astype(np.int64)
    owners = np.unique(rep[rep != np.arange(S)])
    sc = _call((codes, offs), np.stack([owners, owners], 1), mode, matrix, gap_open, gap_extend, unknown, model, "scores")
    ni, na, nc = (np.asarray(_lib.host(v)).astype(np.int64) for v in (sc.n_ident, sc.n_aligned, sc.n_cols))
    denom = (L[owners], na, nc)[thr[2]]
    joins = (denom > 0) & (ni * 10000 >= thr[0] * denom) & (na * 10000 >= thr[1] * L[owners])
    slot = np.full(S, -1, np.int64)
    slot[keep] = np.arange(keep.size)
    joins |= np.bincount(kl, minlength=keep.size)[kl[slot[owners]]] > 1
    joined = np.zeros(S, bool)
    joined[owners] = joins
    key = np.where(joined[rep] | (rep == np.arange(S)), kl[slot[rep]], keep.size + np.arange(S))
    _, firsts, inv = np.unique(key, return_index=True, return_inverse=True)
    full = np.argsort(np.argsort(firsts, kind="stable"), kind="stable")[inv].astype(np.int32)     # numbered by smallest member
    if _lib.is_torch(labels):
        import torch
        return torch.from_numpy(full).to(labels.device)
    return full


def split_clusters(labels, train_ratio=0.8, seed=1337, excluded=None):
    """(train, test, validation) int64 index arrays. The procedure of the reference's split_dataset.ipynb in our words: clusters that hold
    an excluded member go whole to validation; the others, taken in the order of their labels, are shuffled by NumPy's legacy generator
    seeded with ``seed`` (what np.random.seed and np.random.shuffle use) and cut at int(N * train_ratio): the first part trains, the rest
    tests; the members are listed cluster by cluster, ascending within a cluster. excluded: indices or a mask over the sequences."""
    lab = np.asarray(_lib.host(labels)).reshape(-1)
    if lab.size < 1 or not np.issubdtype(lab.dtype, np.integer) or lab.min() < 0:
        raise ValueError("labels must be non-negative integers, one per sequence")
    if not 0.0 <= float(train_ratio) <= 1.0:
        raise ValueError(f"train_ratio must lie in [0, 1], got {train_ratio!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 32:
        raise ValueError(f"seed must be an integer in [0, 2**32), got {seed!r}")
    out = np.zeros(lab.size, bool)
    if excluded is not None:
        e = np.asarray(_lib.host(excluded)).reshape(-1)
        if e.dtype == np.bool_:
            if e.size != lab.size:
                raise ValueError(f"an excluded mask must have {lab.size} entries, got {e.size}")
            out = e.copy()
        elif e.size and (not np.issubdtype(e.dtype, np.integer) or e.min() < 0 or e.max() >= lab.size):
            raise ValueError(f"excluded must hold indices in 0 .. {lab.size - 1} or be a mask")
        else:
            out[e.astype(np.int64)] = True
    ids, inv = np.unique(lab, return_inverse=True)
    order = np.argsort(inv, kind="stable")
    members = np.split(order, np.cumsum(np.bincount(inv))[:-1])
    barred = np.zeros(ids.size, bool)
    barred[inv[out]] = True
    free = [members[c] for c in range(ids.size) if not barred[c]]
    held = [members[c] for c in range(ids.size) if barred[c]]
    pick = np.arange(len(free))
    np.random.RandomState(int(seed)).shuffle(pick)
    n = int(len(free) * float(train_ratio))

    def listed(groups):
        return np.concatenate(groups).astype(np.int64) if groups else np.zeros(0, np.int64)
    return listed([free[c] for c in pick[:n]]), listed([free[c] for c in pick[n:]]), listed(held)


# ------------------------------------------------------------------ structures
def _residues(d):
    """(first atom of every residue int64 [R], chain names [R], one-letter codes uint8 [R], has_ca bool [R]) of a structure dict: a
    residue is a run of equal (chain, resid, icode)"""
    chain = np.asarray(d["chain_name"]).astype(str)
    resid = np.asarray(d["resid"]).astype(np.int64)
    N = resid.size
    if N < 1:
        raise ValueError("a structure has no atoms")
    new = np.ones(N, bool)
    new[1:] = (chain[1:] != chain[:-1]) | (resid[1:] != resid[:-1])
    if "icode" in d:
        ic = np.asarray(d["icode"]).astype(str)
        new[1:] |= ic[1:] != ic[:-1]
    first = np.nonzero(new)[0]
    row = np.cumsum(new) - 1
    has_ca = np.zeros(first.size, bool)
    has_ca[row[np.char.strip(np.asarray(d["name"]).astype(str)) == "CA"]] = True
    if "resname" in d:
        names = np.char.strip(np.asarray(d["resname"]).astype(str)[first])
        codes = encode("".join(THREE_TO_ONE.get(n, "X") for n in names))
    else:
        codes = np.full(first.size, UNKNOWN, np.uint8)
    return first, chain[first], codes, has_ca


def structure_sequences(structure):
    """[(chain_name, codes uint8 [R_c], first-atom index of each residue int64 [R_c])] per protein chain, in the order of first appearance.
    ``structure`` is whatever lddt.structure_lddt takes. A residue is a run of equal (chain, resid, icode); its code is the one-letter
    code of resname for the 20 standard names and X for any other residue that has a CA atom. Residues without a CA are left out, and
    so are chains without any residue of the 20 (ligands, ions, nucleic acids: out of scope)."""
    from .lddt import _structure_dict
    first, chain, codes, has_ca = _residues(_structure_dict(structure))
    out, names = [], []
    for c in chain:
        if c not in names:
            names.append(c)
    for c in names:
        rows = np.nonzero((chain == c) & has_ca)[0]
        if rows.size and np.any(codes[rows] != UNKNOWN):
            out.append((str(c), codes[rows].copy(), first[rows].copy()))
    return out


def match_atoms(reference, predicted, model=None):
    """lddt.match_atoms' five results - (xyz_ref float32 [N, 3], xyz float32 [1, N, 3], res_of_atom int32 [N], chain_of_atom int32 [N],
    table) - with the residues matched by ALIGNMENT instead of by number, so they feed lddt.lddt and tmscore.tm_score unchanged.
    The protein chains of the two structures (structure_sequences) are aligned all against all in one align_scores call ("overlap",
    BLOSUM62, 11 / 1); chains are paired greedily by descending (n_ident, score), then ascending (reference chain, model chain), each
    chain once, and a pairing is kept only with n_ident * 2 >= n_aligned and n_aligned >= 3. The paired chains get one align_maps call;
    within matched residues atoms are matched by name (of duplicates the first counts), NaN where the model lacks the atom, the residue
    or the chain. The reference's atoms stay in their order, all of them (a ligand's too: unmatched, NaN). table: chain_name, resid (and
    resname, icode) of the R residue rows of the reference, resid_model (the model's number of the matched residue, -1 for none) and
    chain_model."""
    return _matched(reference, predicted, model)[:5]


def _matched(reference, predicted, model=None, partner_of=None):
    """partner_of: (a, b, fa, fb) -> the model's residue row under every reference row (structalign.structure_align pairs the residues by
    structure); None: by sequence alignment, as match_atoms states"""
    from .lddt import _structure_dict
    a, b = _structure_dict(reference), _structure_dict(predicted)
    fa, cha, _, _ = _residues(a)
    fb, chb, _, _ = _residues(b)
    N = np.asarray(a["resid"]).size
    ea, eb = np.append(fa, N), np.append(fb, np.asarray(b["resid"]).size)
    sa, sb = structure_sequences(a), structure_sequences(b)
    row_of_a = {int(f): r for r, f in enumerate(fa)}
    row_of_b = {int(f): r for r, f in enumerate(fb)}
    partner = np.full(fa.size, -1, np.int64)            # the model's residue row under every reference row
    if partner_of is not None:
        partner = np.asarray(partner_of(a, b, fa, fb), np.int64)
    elif sa and sb:
        seqs = [s[1] for s in sa] + [s[1] for s in sb]
        na, nb = len(sa), len(sb)
        pairs = np.array([(i, na + j) for i in range(na) for j in range(nb)], np.int32)
        sc = align_scores(seqs, pairs, mode="overlap", model=model)
        ident, score, aligned = (np.asarray(_lib.host(v)).astype(np.int64) for v in (sc.n_ident, sc.score, sc.n_aligned))
        order = np.lexsort((pairs[:, 1], pairs[:, 0], -score, -ident))
        used_a, used_b, chosen = set(), set(), []
        for p in order:
            i, j = int(pairs[p, 0]), int(pairs[p, 1])
            if i in used_a or j in used_b or ident[p] * 2 < aligned[p] or aligned[p] < 3:
                continue
            used_a.add(i)
            used_b.add(j)
            chosen.append(p)
        if chosen:
            chosen = np.sort(np.array(chosen))
            mp = align_maps(seqs, pairs[chosen], mode="overlap", model=model)
            amap = np.asarray(_lib.host(mp.map))
            for q, p in enumerate(chosen):
                i, j = int(pairs[p, 0]), int(pairs[p, 1]) - na
                rows = amap[mp.map_offsets[q]:mp.map_offsets[q + 1]]
                hit = np.nonzero(rows >= 0)[0]
                ra = np.array([row_of_a[int(f)] for f in sa[i][2][hit]], np.int64)
                partner[ra] = [row_of_b[int(f)] for f in sb[j][2][rows[hit]]]
    name_a, name_b = np.asarray(a["name"]).astype(str), np.asarray(b["name"]).astype(str)
    xb = np.asarray(b["xyz"], np.float32).reshape(-1, 3)
    x = np.full((1, N, 3), np.nan, np.float32)
    res = np.zeros(N, np.int32)
    for r in range(fa.size):
        res[ea[r]:ea[r + 1]] = r
        q = partner[r]
        if q < 0:
            continue
        where = {}
        for n in range(eb[q], eb[q + 1]):
            where.setdefault(name_b[n], n)
        for n in range(ea[r], ea[r + 1]):
            k = where.get(name_a[n], -1)
            if k >= 0:
                x[0, n] = xb[k]
    chains = {}
    chain = np.array([chains.setdefault(c, len(chains)) for c in np.asarray(a["chain_name"]).astype(str)], np.int32)
    resid_b = np.asarray(b["resid"]).astype(np.int64)
    table = {"chain_name": cha, "resid": np.asarray(a["resid"]).astype(np.int64)[fa]}
    if "resname" in a:
        table["resname"] = np.asarray(a["resname"]).astype(str)[fa]
    if "icode" in a:
        table["icode"] = np.asarray(a["icode"]).astype(str)[fa]
    table["resid_model"] = np.where(partner >= 0, resid_b[fb[np.maximum(partner, 0)]], -1)
    table["chain_model"] = np.where(partner >= 0, chb[np.maximum(partner, 0)], "")
    return np.ascontiguousarray(np.asarray(a["xyz"], np.float32).reshape(-1, 3)), x, res, chain, table, name_a


def structure_lddt(reference, predicted, mode="all", ca_only=False, thresholds=(0.5, 1, 2, 4), r_incl=15.0, model=None):
    """(Lddt, table): lddt.structure_lddt with the atoms matched by this module's match_atoms (alignment, not residue numbers)."""
    from .lddt import lddt
    y, x, res, chain, table, names = _matched(reference, predicted, model)
    sel = names == "CA" if ca_only else None
    return lddt(y, x, res, chain, mode, sel, thresholds, r_incl, 1.0, model=model), table


def structure_tmscore(reference, predicted, model=None, **kw):
    """(TMScore, table): tmscore.structure_tmscore with the atoms matched by this module's match_atoms. The same argument checks: sel,
    sizes and scale are not taken; at least 3 shared CA atoms."""
    from .tmscore import tm_score
    if "sel" in kw or "sizes" in kw or "scale" in kw:
        raise ValueError("structure_tmscore selects the matched CA atoms itself, in angstroms: sel, sizes and scale are not taken")
    y, x, res, _, table, names = _matched(reference, predicted, model)
    ca = np.char.strip(names) == "CA"
    sel = np.nonzero(ca & np.isfinite(x[0]).all(1))[0]
    kw.setdefault("norm_len", int(ca.sum()) if ca.any() else None)
    if sel.size < 3:
        raise ValueError(f"the two structures share {sel.size} CA atoms: a superposition needs at least 3")
    out = tm_score(y, x, sel, scale=1.0, model=model, **kw)
    rows = res[sel]
    return out, {"chain_name": table["chain_name"][rows], "resid": table["resid"][rows], "resid_model": table["resid_model"][rows],
                 "n_ref": int(ca.sum())}
