"""GPU sweep of pesto_amd.dssp (pesto_dssp.hip) over the seeded cases of tests/dssp_sweep.py (their generators are checked without a GPU by
tests/test_dssp_sweep_fixture.py) against the loop-level definition of tests/golden/make_dssp_golden.py.

Every case goes through compute_dssp(..., return_codes=True) - the codes-only path, which skips the second pair pass - and through
kabsch_sander - the tables-only path, which skips the tail. Everything is compared by equality: codes uint8, partners int32 and
rint(1000 * energies) int32 (energies are float32); there is no tolerance anywhere. Cases run from ROCm tensors; every third case of a kind
also from host arrays, with identical bytes. A case of several structures or frames is also split into one call per structure and one per
frame, which decides an indexing error independently of the definition. The input is unchanged by the call, and a second call gives
identical bits. A failure names the case, frame, structure and local residue and prints the code text around it, or the two table rows."""
import numpy as np
import pytest

import dssp_sweep as S

pytestmark = pytest.mark.gpu
NAMES = ("codes", "partners", "e_m")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def run(X, table, sizes, scale):
    """(codes uint8 [F, R], partners int32 [F, R, 4], e_m int32 [F, R, 4]) as the definition gives them"""
    from pesto_amd import dssp as DS
    codes = DS.compute_dssp(X, table, sizes=sizes, scale=scale, return_codes=True)
    partners, energies = DS.kabsch_sander(X, table, sizes=sizes, scale=scale)
    on_device = hasattr(X, "is_cuda")
    assert all((hasattr(a, "is_cuda") and a.is_cuda) if on_device else isinstance(a, np.ndarray) for a in (codes, partners, energies))
    assert host(energies).dtype == np.float32
    return host(codes), host(partners), np.rint(host(energies).astype(np.float64) * 1000.0).astype(np.int32)


def where(sizes, r):
    """(structure, local residue) of residue r of the batch"""
    offs = np.cumsum([0] + list(sizes))
    s = int(np.searchsorted(offs, r, side="right")) - 1
    return s, r - int(offs[s])


def compare(case, what, sizes, got, want):
    """equality of (codes, partners, e_m), each [F, R (, 4)]; the message locates the first difference"""
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (S.case_id(case), what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        if bad.size == 0:
            continue
        f, r = int(bad[0][0]), int(bad[0][1])
        s, l = where(sizes, r)
        offs = np.cumsum([0] + list(sizes))
        head = f"{S.case_id(case)} [{what}]: {name} differ at frame {f}, structure {s} ({sizes[s]} residues), local residue {l} ({len(bad)} entries differ)"
        if name == "codes":
            lo, hi = max(int(offs[s]), r - 10), min(int(offs[s + 1]), r + 11)
            raise AssertionError(f"{head}\n  residues {lo - offs[s]} .. {hi - 1 - offs[s]}\n  got  {S.text(g[f, lo:hi])!r}\n  want {S.text(w[f, lo:hi])!r}")
        raise AssertionError(f"{head}\n  got  partners {got[1][f, r].tolist()} e_m {got[2][f, r].tolist()}\n"
                             f"  want partners {want[1][f, r].tolist()} e_m {want[2][f, r].tolist()}")


def same_bits(a, b):
    return all(u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes() for u, v in zip(a, b))


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_case_equals_the_definition(case):
    c = S.build(case)
    X, sizes, scale = c["X"], c["sizes"], c["scale"]
    table = (c["table"], c["pro"], c["chain"])
    want = (c["codes"], c["partners"], c["em"])
    F = X.shape[0]
    x = dev(X)
    got = run(x, table, sizes, scale)
    compare(case, "ROCm tensor", sizes, got, want)
    assert host(x).tobytes() == X.tobytes(), (S.case_id(case), "the input tensor changed")
    assert same_bits(run(x, table, sizes, scale), got), (S.case_id(case), "a second call gives other bits")
    if S.every_third(case):
        keep = X.copy()
        from_host = run(X, table, sizes, scale)
        compare(case, "host arrays", sizes, from_host, want)
        assert same_bits(from_host, got) and X.tobytes() == keep.tobytes(), (S.case_id(case), "host against device")
    # the same call one structure at a time, and one frame at a time: the kernels' (frame, structure) offsets against themselves
    if len(sizes) > 1:
        offs = np.cumsum([0] + sizes)
        parts = [run(x, tuple(t[offs[s]:offs[s + 1]] for t in table), None, scale) for s in range(len(sizes))]
        compare(case, "one call per structure against the batch", sizes, tuple(np.concatenate([p[k] for p in parts], 1) for k in range(3)), got)
    if F > 1:
        parts = [run(x[f:f + 1], table, sizes, scale) for f in range(F)]
        compare(case, "one call per frame against all frames", sizes, tuple(np.concatenate([p[k] for p in parts], 0) for k in range(3)), got)
