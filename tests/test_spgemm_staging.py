"""Device SpGEMM at the places where its row staging can go wrong.

The wave-per-row tiers stage a row's A entries with all 64 lanes (a wave scan
per 64-entry chunk, the total carried across chunks); the 8-lanes-per-row
tier stages 8 A entries at a time, and its count pass flattens their
products over the lanes.  Every case here is a
few hundred rows built so that a named length lands exactly on a boundary of
that code: chunk widths (8, 64), BIGROW (256), SGSMALL (ub 96/97), the fill
tiers (output length 20/21, 48/49, 96/97).  `test_cases_hit_the_boundaries`
checks the constructed lengths on the host; the GPU tests compare
`spgemm(sort=True)` and `spgemm(sort=False)` with SciPy's product.
"""
import numpy as np
import pytest
import scipy.sparse as sp

SGSMALL = 96
BIGROW = 256


@pytest.fixture(scope="module")
def hip():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from amgcl_amd.backend import make_backend

    return make_backend("hip")


def _csr(rows, ncols, rng):
    """CSR with the given column list per row and seeded normal values."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    assert all(len(set(r)) == len(r) for r in rows)
    m = sp.csr_matrix((rng.standard_normal(len(col)), col, ptr),
                      shape=(len(rows), ncols))
    m.sort_indices()
    return m


def _ub(A, B):
    """Per-row product upper bound, as the device bins rows."""
    blen = np.diff(B.indptr)
    return np.array([blen[A.indices[A.indptr[i]:A.indptr[i + 1]]].sum()
                     for i in range(A.shape[0])])


def _pick(rng, pool, n):
    return sorted(rng.choice(pool, size=n, replace=False).tolist())


def case_wave_staging():
    """alen 1..257 with ub > SGSMALL: chunk carry, BIGROW, and the huge path."""
    rng = np.random.default_rng(101)
    m, k = 300, 400
    brows = [_pick(rng, k, 100)]                     # one long row for alen 1
    brows += [_pick(rng, k, int(rng.integers(2, 5))) for _ in range(m - 1)]
    alens = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    arows = [[0]] + [_pick(rng, np.arange(1, m), a) for a in alens[1:]]
    arows += [_pick(rng, np.arange(1, m), int(a)) for a in rng.integers(40, 200, 30)]
    return _csr(arows, m, rng), _csr(brows, k, rng), alens


def case_empty_b_rows():
    """Empty B rows at the start, the end and in runs inside staged rows
    (repeated prefix values), plus empty A rows."""
    rng = np.random.default_rng(102)
    m, k, nempty = 200, 300, 60
    brows = [[] for _ in range(nempty)]
    brows += [_pick(rng, k, int(rng.integers(3, 6))) for _ in range(m - nempty)]
    E = list(range(nempty))
    F = list(range(nempty, m))

    def mixed(pattern):
        # pattern: list of (is_empty, count), in the A row's storage order
        e, f, out = iter(rng.permutation(E)), iter(rng.permutation(F)), []
        for is_empty, cnt in pattern:
            out += [int(next(e if is_empty else f)) for _ in range(cnt)]
        return out

    arows = [
        [],                                                         # empty A row
        mixed([(1, 5), (0, 20), (1, 6), (0, 25), (1, 1), (0, 9), (1, 4)]),  # alen 70
        mixed([(1, 3), (0, 58), (1, 6), (0, 30), (1, 2)]),          # empties over 62..66
        mixed([(0, 30), (1, 10)]),                                  # alen 40
        [],
        mixed([(1, 2), (0, 1), (1, 3), (0, 2), (1, 1)]),            # small tier, alen 9
        mixed([(1, 8), (0, 1)]),                                    # a chunk of empties
        mixed([(0, 1), (1, 8), (0, 8), (1, 1)]),
        mixed([(1, 7)]),                                            # ub = 0
        [],
    ]
    # A rows keep the order given (unsorted columns are legal for the product)
    ptr = np.zeros(len(arows) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(r) for r in arows])
    col = np.array([c for r in arows for c in r], dtype=np.int32)
    A = sp.csr_matrix((rng.standard_normal(len(col)), col, ptr),
                      shape=(len(arows), m))
    return A, _csr(brows, k, rng)


def case_small_tier():
    """A lengths 1, 7, 8, 9, 16, 17 over B rows of length 0, 1, 8, 9, and
    ub exactly SGSMALL and SGSMALL + 1."""
    rng = np.random.default_rng(103)
    k, per = 60, 20
    blens = [0, 1, 8, 9]
    brows = [_pick(rng, k, L) for L in blens for _ in range(per)]
    rows_of = {L: list(range(i * per, (i + 1) * per)) for i, L in enumerate(blens)}
    alens = [1, 7, 8, 9, 16, 17]
    arows = []
    for a in alens:
        for order in ([1, 8, 0, 9], [0, 9, 1, 8], [1, 1, 1, 1], [8, 0, 0, 1]):
            used = {L: 0 for L in blens}
            r = []
            for j in range(a):
                L = order[j % 4]
                r.append(rows_of[L][used[L]])
                used[L] += 1
            arows.append(r)
    arows.append(rows_of[8][:12])                     # ub = 96: small tier
    arows.append(rows_of[8][:11] + rows_of[9][:1])    # ub = 97: wave tier
    A = _csr(arows, len(brows), rng)
    return A, _csr(brows, k, rng), alens


def case_fill_tiers():
    """Exact output lengths on both sides of every fill tier.  B rows have
    disjoint column ranges, so the output length is the sum of the B-row
    lengths; rows d6/d6' and d7/d7' repeat a range so that a wave-tier row
    (ub > SGSMALL) can have 96 or 97 distinct columns."""
    rng = np.random.default_rng(104)
    blens = [10] * 9 + [1, 8, 9, 6, 7]
    brows, c = [], 0
    for L in blens:
        brows.append(list(range(c, c + L)))
        c += 16
    i1, i8, i9, i6, i7 = 9, 10, 11, 12, 13
    brows += [list(brows[i6]), list(brows[i7])]       # d6', d7'
    i6b, i7b = 14, 15
    ten = list(range(9))
    arows = [
        ten[:2],                       # len 20  -> 32-slot fill
        ten[:2] + [i1],                # len 21  -> 64-slot fill
        ten[:4] + [i8],                # len 48  -> 64-slot fill
        ten[:4] + [i9],                # len 49  -> 128-slot small fill
        ten + [i6, i6b],               # ub 102, len 96 -> wave tier, 128 slots
        ten + [i7, i7b],               # ub 104, len 97 -> wave tier, 512 slots
        ten + [i7],                    # ub 97,  len 97
        ten + [i6],                    # ub 96,  len 96 -> small tier
    ]
    want = [20, 21, 48, 49, 96, 97, 97, 96]
    return _csr(arows, len(brows), rng), _csr(brows, c, rng), want


def case_duplicates():
    """Many A entries whose B rows share the same six columns."""
    rng = np.random.default_rng(105)
    m = 300
    hot = [3, 17, 64, 65, 200, 511]
    brows = [_pick(rng, hot, int(rng.integers(2, 4))) for _ in range(m)]
    alens = [5, 17, 30, 100, 256, 300]
    arows = [_pick(rng, m, a) for a in alens]
    return _csr(arows, m, rng), _csr(brows, 512, rng), alens


CASES = {
    "wave_staging": lambda: case_wave_staging()[:2],
    "empty_b_rows": case_empty_b_rows,
    "small_tier": lambda: case_small_tier()[:2],
    "fill_tiers": lambda: case_fill_tiers()[:2],
    "duplicates": lambda: case_duplicates()[:2],
}


@pytest.fixture(scope="module")
def refs():
    """Inputs and the SciPy product of every case, computed once."""
    out = {}
    for name, make in CASES.items():
        A, B = make()
        C = (A @ B).tocsr()
        C.sort_indices()
        out[name] = (A, B, C)
    return out


def test_cases_hit_the_boundaries():
    A, B, alens = case_wave_staging()
    assert np.diff(A.indptr)[:len(alens)].tolist() == alens
    assert alens[-2] == BIGROW and alens[-1] == BIGROW + 1
    assert (_ub(A, B) > SGSMALL).all()
    assert np.diff((A @ B).tocsr().indptr).max() < 448   # LDS hash capacity

    A, B = case_empty_b_rows()
    alen, ub, blen = np.diff(A.indptr), _ub(A, B), np.diff(B.indptr)
    assert (alen == 0).sum() == 3
    assert alen[1] == 70 and alen[2] == 99 and (ub[1:4] > SGSMALL).all()
    assert (blen[A.indices[A.indptr[1]:A.indptr[1] + 5]] == 0).all()       # start
    assert (blen[A.indices[A.indptr[2] - 4:A.indptr[2]]] == 0).all()       # end
    assert (blen[A.indices[A.indptr[2] + 61:A.indptr[2] + 67]] == 0).all()  # 61..66
    assert (ub[5:9] <= SGSMALL).all() and ub[8] == 0

    A, B, alens = case_small_tier()
    assert sorted(set(np.diff(B.indptr))) == [0, 1, 8, 9]
    assert set(alens) <= set(np.diff(A.indptr))
    ub = _ub(A, B)
    assert ub[-2] == SGSMALL and ub[-1] == SGSMALL + 1
    assert (ub[:-1] <= SGSMALL).all()

    A, B, want = case_fill_tiers()
    assert np.diff((A @ B).tocsr().indptr).tolist() == want
    assert _ub(A, B).tolist() == [20, 21, 48, 49, 102, 104, 97, 96]

    A, B, alens = case_duplicates()
    assert np.diff(A.indptr).tolist() == alens
    ub = _ub(A, B)
    assert (ub[:3] <= SGSMALL).all() and (ub[3:] > SGSMALL).all()
    assert np.diff((A @ B).tocsr().indptr).max() <= 6


def _check(hip, A, B, ref):
    from amgcl_amd.backend import hip_setup
    from amgcl_amd.matrix import CSR

    n, k = ref.shape
    Ad = hip.matrix(CSR(A.shape[0], A.shape[1], A.indptr, A.indices, A.data))
    Bd = hip.matrix(CSR(B.shape[0], B.shape[1], B.indptr, B.indices, B.data))
    rows = np.repeat(np.arange(n), np.diff(ref.indptr))
    for sort in (True, False):
        Cd = hip_setup.spgemm(Ad, Bd, sort=sort)
        ptr = Cd.ptr.cpu().numpy()
        col = Cd.col.cpu().numpy().astype(np.int64)
        val = Cd.val.cpu().numpy()
        np.testing.assert_array_equal(ptr, ref.indptr, err_msg=f"sort={sort}")
        assert col.shape == ref.indices.shape
        if sort:
            # ascending within each row and the exact column set, at once
            np.testing.assert_array_equal(col, ref.indices)
            order = np.arange(len(col))
        else:
            order = np.lexsort((col, rows))
            np.testing.assert_array_equal(col[order], ref.indices)
        np.testing.assert_allclose(val[order], ref.data, rtol=1e-12, atol=1e-13,
                                   err_msg=f"sort={sort}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_spgemm_staging(hip, refs, name):
    _check(hip, *refs[name])


@pytest.mark.gpu
def test_galerkin_end_to_end(hip):
    import amgcl_amd as am
    from amgcl_amd.backend import hip_setup
    from amgcl_amd.backend.hip_setup import poisson3d_device
    from amgcl_amd.matrix import galerkin

    n = 24
    Ad = poisson3d_device(n)
    A, _ = am.poisson3d(n)
    naggr, ids, strong = hip_setup.aggregates(Ad, 0.08)
    P = hip_setup.smoothed_prolongation(Ad, strong, ids, naggr, 2.0 / 3.0)
    R = hip_setup.transpose(P)
    Ac = hip_setup.download(galerkin(R, Ad, P)).to_scipy()
    P_h = hip_setup.download(P)
    Ac_h = (P_h.transpose() @ (A @ P_h)).to_scipy()
    assert Ac.shape == Ac_h.shape
    assert abs(Ac - Ac_h).max() < 1e-11
