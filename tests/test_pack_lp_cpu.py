"""capi.pack_lp, the one place the binding turns an LP's arrays into the ABI's form: shapes, dtypes and bytes for one
LP and for a batch, and a ValueError for every array that is one entry short.  Pure numpy: no context, no library."""
import numpy as np
import pytest

from simplexmethod_amd import capi

M, N, B = 3, 5, 4


def _lp(batch=None, seed=0):
    rng = np.random.default_rng(seed)
    lead = () if batch is None else (batch,)
    return dict(A=rng.standard_normal(lead + (M, N)), b=rng.standard_normal(lead + (M,)),
                c=rng.standard_normal(lead + (N,)), basis=rng.integers(0, N, lead + (M,)),
                lo=rng.standard_normal(lead + (N,)), hi=rng.standard_normal(lead + (N,)),
                at_upper=rng.integers(0, 2, lead + (N,)))


def _check_flat(out, lp, batch):
    names = ("b", "c", "basis", "lo", "hi", "at_upper")
    for name, v in zip(names, out[4:]):
        want = np.int32 if name in ("basis", "at_upper") else np.float64
        assert v.dtype == want and v.ndim == 1 and v.flags["C_CONTIGUOUS"], name
        assert v.size == batch * (M if name in ("b", "basis") else N), name
        assert np.array_equal(v, np.asarray(lp[name]).reshape(-1)), name


def test_single_lp():
    lp = _lp()
    out = capi.pack_lp(**lp)
    assert out._fields == ("batch", "m", "n", "A", "b", "c", "basis", "lo", "hi", "at_upper")
    assert out.lo is out[7] and out.hi is out[8] and out.basis is out[6] and out.at_upper is out[9]
    assert len(out) == 10 and out[:3] == (1, M, N)
    Af = out[3]
    assert Af.dtype == np.float64 and Af.shape == (M * N,) and Af.flags["C_CONTIGUOUS"]
    assert Af.tobytes() == capi.colmajor(lp["A"]).tobytes()
    assert np.array_equal(Af.reshape(N, M), lp["A"].T)   # column j of A is Af[j*M:(j+1)*M]
    _check_flat(out, lp, 1)


def test_batched():
    lp = _lp(B)
    out = capi.pack_lp(**lp, batched=True)
    assert len(out) == 10 and out[:3] == (B, M, N)
    Af = out[3]
    assert Af.dtype == np.float64 and Af.shape == (B * M * N,) and Af.flags["C_CONTIGUOUS"]
    assert Af.tobytes() == np.ascontiguousarray(np.transpose(lp["A"], (0, 2, 1))).tobytes()
    for k in range(B):
        assert Af[k * M * N:(k + 1) * M * N].tobytes() == capi.colmajor(lp["A"][k]).tobytes()
    _check_flat(out, lp, B)


def test_what_is_not_given_stays_none():
    lp = _lp()
    out = capi.pack_lp(lp["A"], lp["b"], lp["c"])
    assert out[6:] == (None, None, None, None)
    out = capi.pack_lp(lp["A"], lp["b"], lp["c"], lo=lp["lo"], hi=lp["hi"])
    assert out[6] is None and out[9] is None and out[7].size == N and out[8].size == N


@pytest.mark.parametrize("batch", [None, B])
def test_layout_and_dtype_of_the_input_do_not_matter(batch):
    lp = _lp(batch, seed=1)
    kw = dict(batched=batch is not None)
    ref = capi.pack_lp(**lp, **kw)
    # Fortran-ordered A: the same values, so the same bytes as the C-ordered one
    assert capi.pack_lp(**dict(lp, A=np.asfortranarray(lp["A"])), **kw)[3].tobytes() == ref[3].tobytes()
    # float32 A: the bytes of its float64 widening; nested lists and int64 / bool index arrays likewise
    A32 = lp["A"].astype(np.float32)
    wide = capi.pack_lp(**dict(lp, A=A32.astype(np.float64)), **kw)[3]
    assert capi.pack_lp(**dict(lp, A=A32), **kw)[3].tobytes() == wide.tobytes()
    loose = capi.pack_lp(lp["A"].tolist(), lp["b"].tolist(), lp["c"][..., ::-1][..., ::-1],
                         lp["basis"].astype(np.int64), lp["lo"], lp["hi"], lp["at_upper"].astype(bool), **kw)
    for got, want in zip(loose[3:], ref[3:]):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("batch", [None, B])
@pytest.mark.parametrize("name", ["b", "c", "lo", "hi", "basis", "at_upper"])
def test_one_entry_short_is_refused(name, batch):
    lp = _lp(batch, seed=2)
    capi.pack_lp(**lp, batched=batch is not None)
    lp[name] = np.asarray(lp[name]).reshape(-1)[:-1]
    with pytest.raises(ValueError, match=name):
        capi.pack_lp(**lp, batched=batch is not None)


def test_a_of_the_wrong_rank_is_refused():
    lp = _lp()
    with pytest.raises(ValueError):
        capi.pack_lp(**lp, batched=True)
    with pytest.raises(ValueError):
        capi.pack_lp(**_lp(B))


def test_batched_is_by_keyword_only():
    with pytest.raises(TypeError):
        capi.pack_lp(*_lp(B).values(), True)


@pytest.mark.parametrize("size", [M, B * N])
def test_direction_one_entry_short_is_refused(size):
    v = np.arange(size, dtype=np.float32).reshape(-1, M if size == M else N)
    d = capi._direction(v, size)
    assert d.dtype == np.float64 and d.shape == (size,) and np.array_equal(d, np.arange(size))
    with pytest.raises(ValueError, match=f"must have {size} entries, got {size - 1}"):
        capi._direction(v.reshape(-1)[:-1], size)
    with pytest.raises(ValueError, match=f"^parametric: expected {size} direction entries, got {size - 1}$"):
        capi._direction(v.reshape(-1)[:-1], size, "parametric: expected {size} direction entries, got {got}")
