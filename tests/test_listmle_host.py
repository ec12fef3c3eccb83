"""CPU tier of ListMLE (include/ltr_listwise.h, pytorchltr_amd.loss.ListMLELoss): the fp64 oracle against the definition,
finite differences and torch.autograd, the C ABI's table, return codes and workspace sizes, and the new kernels'
register use.  Parity is unpinned (the reference has no ListMLE): the header is the specification."""
import ctypes
import math
import os

import numpy as np
import pytest

# ---- the oracle: an fp64 restatement of include/ltr_listwise.h ----


def oracle_order(y, nb, tie=None):
    """pi of one row: the first nb documents by label (compared as fp32), descending; equal labels by ascending tie
    word (`tie`: (>= nb) unsigned words, None: document index)."""
    lab = np.asarray(y[:nb], dtype=np.float32).astype(np.float64)
    words = np.arange(nb, dtype=np.int64) if tie is None else np.asarray(tie[:nb]).astype(np.uint32).astype(np.int64)
    return np.lexsort((words, -lab))


def oracle(s, y, n, k=None, tie=None):
    """(loss (B,), dscores (B, L)) in fp64.  `tie`: (L) tie words shared by every row, or None for index order."""
    s = np.asarray(s, dtype=np.float64)
    B, L = s.shape
    loss, ds = np.zeros(B), np.zeros((B, L))
    for b in range(B):
        nb = int(min(max(int(n[b]), 0), L))
        if nb == 0:
            continue
        pi = oracle_order(y[b], nb, tie)
        x = s[b, pi]
        K = nb if k is None else min(int(k), nb)
        lse = np.logaddexp.accumulate(x[::-1])[::-1]                   # LSE_m = log sum_{i >= m} exp(x_i)
        loss[b] = np.sum(lse[:K] - x[:K])
        first = (np.arange(nb) < K).astype(np.float64)
        d = np.zeros(nb)                                               # D_i = [i < K] + D_{i-1} exp(LSE_i - LSE_{i-1})
        prev = 0.0
        for i in range(nb):
            prev = first[i] + (prev * math.exp(lse[i] - lse[i - 1]) if i > 0 else 0.0)
            d[i] = prev
        ds[b, pi] = np.exp(x - lse) * d - first
    return loss, ds


def definition(s, y, n, k=None, tie=None):
    """The loss term by term in python floats: sum_{m < K} (log sum_{i >= m} exp(x_i) - x_m)."""
    out = []
    for b in range(s.shape[0]):
        nb = max(0, min(int(n[b]), s.shape[1]))
        pi = oracle_order(y[b], nb, tie)
        x = [float(s[b, j]) for j in pi]
        K = nb if k is None else min(k, nb)
        out.append(sum(math.log(sum(math.exp(v) for v in x[m:])) - x[m] for m in range(K)))
    return np.array(out)


def torch_composition(s, y, n, k=None):
    """The same definition as a torch program (index ties): stable argsort of the labels, gather, logcumsumexp on the
    flipped list, autograd.  fp64 on the CPU; returns (loss, dscores) of loss.sum()."""
    import torch
    st = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(np.asarray(y, dtype=np.float32), dtype=torch.float64)
    nt = torch.tensor(n, dtype=torch.int64).clamp(0, s.shape[1])
    L = s.shape[1]
    pos = torch.arange(L).unsqueeze(0)
    real = pos < nt.unsqueeze(1)
    key = torch.where(real, yt, torch.full_like(yt, -math.inf))
    pi = torch.sort(key, dim=1, descending=True, stable=True).indices
    x = torch.gather(st, 1, pi)
    x = torch.where(real, x, torch.full_like(x, -math.inf))
    lse = torch.flip(torch.logcumsumexp(torch.flip(x, [1]), 1), [1])
    K = nt if k is None else nt.clamp(max=k)
    take = pos < K.unsqueeze(1)
    loss = torch.where(take, lse - torch.where(real, x, torch.zeros_like(x)), torch.zeros_like(x)).sum(1)
    loss.sum().backward()
    return loss.detach().numpy(), st.grad.numpy()


def _batch(seed, B, L, float_labels=False, grades=5):
    rng = np.random.default_rng(seed)
    s = rng.normal(0.0, 2.0, (B, L))
    y = rng.uniform(0, 3, (B, L)) if float_labels else rng.integers(0, grades, (B, L))
    n = rng.integers(0, L + 1, B)
    for i, v in enumerate((0, 1, L, L + 5)):
        if i < B:
            n[i] = v
    return s, y, n


@pytest.mark.parametrize("k", [None, 1, 3, 9, 40])
@pytest.mark.parametrize("float_labels", [False, True])
def test_oracle_matches_the_definition_and_torch(k, float_labels):
    s, y, n = _batch(1, 7, 9, float_labels)
    loss, ds = oracle(s, y, n, k)
    assert np.allclose(loss, definition(s, y, n, k), rtol=1e-12, atol=1e-12)
    tl, tg = torch_composition(s, y, n, k)
    assert np.allclose(loss, tl, rtol=1e-12, atol=1e-12)
    assert np.allclose(ds, tg, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("k", [None, 1, 3])
def test_oracle_matches_finite_differences(k):
    s, y, n = _batch(2, 5, 8)
    loss, ds = oracle(s, y, n, k)
    eps = 1e-6
    for b in range(s.shape[0]):
        for j in range(s.shape[1]):
            sp, sm = s.copy(), s.copy()
            sp[b, j] += eps
            sm[b, j] -= eps
            fd = (oracle(sp, y, n, k)[0][b] - oracle(sm, y, n, k)[0][b]) / (2 * eps)
            assert abs(fd - ds[b, j]) < 1e-7, (b, j)


def test_oracle_edges_shift_invariance_and_zero_row_sums():
    s, y, n = _batch(3, 6, 12)
    loss, ds = oracle(s, y, n)
    assert loss[0] == 0.0 and np.all(ds[0] == 0.0)                     # n = 0
    assert loss[1] == 0.0 and np.all(ds[1] == 0.0)                     # n = 1: one factor, probability 1
    assert np.allclose(ds.sum(1), 0.0, atol=1e-12)                     # sum_j dscores[b, j] = 0 on every row
    for k in (None, 1, 4):
        l0, d0 = oracle(s, y, n, k)
        l1, d1 = oracle(s + 1000.0, y, n, k)
        assert np.allclose(l0, l1, rtol=1e-9, atol=1e-9) and np.allclose(d0, d1, atol=1e-9)
        assert np.allclose(d0.sum(1), 0.0, atol=1e-12)
    # padded slots take no part
    s2, y2 = s.copy(), y.copy()
    for b in range(s.shape[0]):
        s2[b, n[b]:] = 1e6
        y2[b, n[b]:] = 99
    l2, d2 = oracle(s2, y2, n)
    assert np.array_equal(l2, loss) and np.array_equal(d2, ds)


def test_oracle_all_tied_labels_follow_the_tie_words():
    rng = np.random.default_rng(4)
    s, y, n = rng.normal(size=(3, 10)), np.zeros((3, 10), dtype=np.int64), np.array([10, 7, 10])
    words = rng.permutation(10).astype(np.uint32)
    loss, ds = oracle(s, y, n, tie=words)
    order = np.argsort(words[:10], kind="stable")
    x = s[0, order]
    want = sum(math.log(sum(math.exp(v) for v in x[m:])) - x[m] for m in range(10))
    assert loss[0] == pytest.approx(want, rel=1e-12)
    # index order is a different ranking, so a different loss
    assert oracle(s, y, n)[0][0] != pytest.approx(loss[0], rel=1e-9)


def test_oracle_large_spread_is_finite():
    rng = np.random.default_rng(5)
    s = rng.uniform(-200, 200, (4, 50))
    y = rng.integers(0, 5, (4, 50))
    loss, ds = oracle(s, y, np.array([50, 30, 2, 49]))
    assert np.all(np.isfinite(loss)) and np.all(np.isfinite(ds))


# ---- the Python module, no GPU ----


def test_module_arguments_and_exports():
    import torch
    from pytorchltr_amd import loss as L
    assert "ListMLELoss" in L.__all__ and L.ListMLELoss is L.listwise.ListMLELoss
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError):
            L.ListMLELoss(k=bad)
    assert L.ListMLELoss().state_dict() == {} and list(L.ListMLELoss(k=4).parameters()) == []
    assert L.ListMLELoss(k=4).k == 4 and L.ListMLELoss().k is None
    with pytest.raises(RuntimeError):                                  # no CPU fallback
        L.ListMLELoss()(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 3]))


# ---- include/ltr_listwise.h: table, return codes, workspace sizes (no case below gets as far as a launch) ----

P = 256                                        # dummy non-NULL device pointer: never dereferenced below
_ARGS = ["scores", "rel", "rel_dtype", "n", "k", "tie", "use_seed", "seed", "seed_dev", "B", "L", "loss", "dscores",
         "workspace", "workspace_bytes", "stream"]
_VALID = dict(scores=P, rel=P, rel_dtype=0, n=P, k=0, tie=None, use_seed=0, seed=0, seed_dev=None, B=2, L=16, loss=P,
              dscores=P, workspace=P, workspace_bytes=1 << 40, stream=None)
LONG = dict(L=5000)                            # past 4096 documents: the sort path, which needs the workspace

CASES = [
    (dict(scores=None), -1), (dict(rel=None), -1), (dict(n=None), -1), (dict(loss=None), -1),
    (dict(B=-1), -2), (dict(B=0), 0), (dict(B=0, scores=None), 0), (dict(L=0), -2), (dict(L=-5), -2),
    (dict(L=(1 << 24) + 1), -4), (dict(rel_dtype=7), -3), (dict(rel_dtype=-1), -3),
    (dict(LONG, workspace_bytes=1), -5), (dict(LONG, workspace=None), -5), (dict(LONG, workspace_bytes=0), -5),
    # two at once: dtype, then the lists, then NULL, then the workspace
    (dict(rel_dtype=7, B=-1), -3), (dict(rel_dtype=7, scores=None), -3), (dict(L=0, loss=None), -2),
    (dict(L=(1 << 24) + 1, scores=None), -4), (dict(LONG, workspace=None, n=None), -1),
    (dict(LONG, workspace_bytes=1, B=0), 0),
]


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    if not os.environ.get("LTR_HIP_LIB"):
        build_extension()
    return _C.lib()


@pytest.mark.parametrize("i", range(len(CASES)))
def test_listmle_return_codes(lib, i):
    change, want = CASES[i]
    args = dict(_VALID, **change)
    assert lib.ltr_listmle_f32(*[args[a] for a in _ARGS]) == want, change


def test_listmle_workspace_bytes(lib):
    ws = lib.ltr_listmle_workspace_bytes
    al = lambda x: -(-x // 256) * 256                                  # noqa: E731
    for L in (1, 16, 128, 4096):
        assert ws(3, L) == 0, L                                        # one workgroup per query: none
    for B, L in ((2, 4097), (2, 5000), (4, 200000)):
        tiles = -(-L // 4096)
        assert ws(B, L) == al(16 * B * L) + al(4 * L) + 3 * al(4 * B * L) + al(16 * B * tiles) + 4 * B * tiles
    for bad in [(-1, 5000), (2, 0), (2, -1), (2, (1 << 24) + 1)]:
        assert ws(*bad) == 0, bad
    prev = lib.ltr_debug_long_sort_all(1)                              # the forced sort path needs it at any L
    try:
        assert ws(2, 16) == al(16 * 2 * 16) + al(4 * 16) + 3 * al(4 * 2 * 16) + al(16 * 2) + 4 * 2
    finally:
        lib.ltr_debug_long_sort_all(prev)


@pytest.mark.parametrize("B", [1, 24])
def test_listmle_workspace_bytes_grid(lib, B):
    """The header's byte formula where the tile and chunk counts change (one tile more at 4097, 8193; several at 20000):
    the workspace is stated once, as a carving, and its size must stay what the header says."""
    ws = lib.ltr_listmle_workspace_bytes
    al = lambda x: -(-x // 256) * 256                                  # noqa: E731
    for L in (1, 256, 4095, 4096):
        assert ws(B, L) == 0, L
    for L in (4097, 8192, 8193, 20000):
        tiles = -(-L // 4096)
        assert ws(B, L) == al(16 * B * L) + al(4 * L) + 3 * al(4 * B * L) + al(16 * B * tiles) + 4 * B * tiles, L


def test_listmle_header_matches_the_ctypes_table(lib):
    import re
    from pytorchltr_amd import _C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ltr_listwise.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(ltr_[a-z0-9_]+)\s*\(", text))) == sorted(_C.LISTWISE_SIGNATURES)
    assert not set(_C.LISTWISE_SIGNATURES) & (set(_C.SIGNATURES) | set(_C.EVAL_SIGNATURES))
    for name in _C.LISTWISE_SIGNATURES:                                # exported by the library
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name


def test_listmle_kernels_do_not_spill():
    """tests/test_codeobj.py's rule for the new kernels: no VGPR spill, no scratch."""
    from pytorchltr_amd import _codeobj
    from pytorchltr_amd.build import LIB_PATH, build_extension
    build_extension()
    try:
        recs = _codeobj.kernel_records(LIB_PATH)
    except FileNotFoundError as exc:          # no llvm tools on this machine
        pytest.skip(str(exc))
    names = [r.get("demangled", r["name"]) for r in recs]
    ours = [r for r, n in zip(recs, names) if "listmle_" in n or ("longsort_chunk_kernel<" in n and ", 1>" in n)]
    assert len(ours) == 12, names                                      # 6 one-workgroup shapes, 5 tile kernels, 1 key sort
    for r in ours:
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r.get("demangled")
