"""CPU tier: the long-list entry points (include/ltr_hip.h: ltr_*_long_f32) -- argument validation decided on the
host before any launch, the workspace formula, and the long tie word against its numpy restatement."""
import numpy as np
import pytest

# dummy non-NULL device pointers: every call below returns before it would launch
P = 256


@pytest.fixture(scope="module")
def lib():
    from pytorchltr_amd import _C
    from pytorchltr_amd.build import build_extension
    build_extension()
    return _C.lib()


def _rank(lib, B, L, ws=None, nbytes=0, scores=P, n=P, out=P):
    return lib.ltr_rank_by_score_long_f32(scores, n, None, 0, 0, None, B, L, out, ws, nbytes, None)


def _dcg(lib, B, L, k=10, ws=None, nbytes=0, scores=P, rel=P, n=P, out=P, dtype=0):
    return lib.ltr_dcg_long_f32(scores, rel, dtype, n, None, 0, 0, None, B, L, k, 1, 1, out, ws, nbytes, None)


def _arp(lib, B, L, ws=None, nbytes=0, scores=P, rel=P, n=P, out=P, dtype=0):
    return lib.ltr_arp_long_f32(scores, rel, dtype, n, None, 0, 0, None, B, L, out, ws, nbytes, None)


def test_bounds(lib):
    assert lib.ltr_max_sort_list_len() >= 1 << 20
    assert lib.ltr_max_list_len() == 4096


def test_argument_validation(lib):
    M = lib.ltr_max_sort_list_len()
    L = 5000
    # a missing pointer
    assert _rank(lib, 2, L, scores=None) == -1
    assert _rank(lib, 2, L, out=None) == -1
    assert _rank(lib, 2, L, n=None) == -1
    assert _dcg(lib, 2, L, rel=None) == -1
    assert _dcg(lib, 2, L, out=None) == -1
    assert _arp(lib, 2, L, scores=None) == -1
    assert _arp(lib, 2, L, n=None) == -1
    # bad B, L or k
    for fn in (_rank, _dcg, _arp):
        assert fn(lib, -1, L) == -2
        assert fn(lib, 2, 0) == -2
    assert _dcg(lib, 2, L, k=-1) == -2
    # bad label dtype
    assert _dcg(lib, 2, L, dtype=7) == -3
    assert _arp(lib, 2, L, dtype=7) == -3
    # too long
    for fn in (_rank, _dcg, _arp):
        assert fn(lib, 2, M + 1) == -4
        assert fn(lib, 0, M + 1) == -4
    # no queries: nothing to do
    for fn in (_rank, _dcg, _arp):
        assert fn(lib, 0, L, scores=None) == 0
    # missing or short workspace on the long path
    for op, fn in ((0, _rank), (1, _dcg), (2, _arp)):
        need = lib.ltr_sort_workspace_bytes(op, 2, L)
        assert need > 0
        assert fn(lib, 2, L) == -5
        assert fn(lib, 2, L, ws=P, nbytes=need - 1) == -5
        assert fn(lib, 2, M, ws=P, nbytes=lib.ltr_sort_workspace_bytes(op, 2, M) - 1) == -5


def test_workspace_formula(lib):
    for op in (0, 1, 2):
        prev_b = 0
        for B in (1, 2, 7, 64, 1000):
            prev_l = 0
            for L in (1, 100, 4096, 4097, 8192, 8193, 100000, 1 << 22):
                w = lib.ltr_sort_workspace_bytes(op, B, L)
                assert w >= 16 * B * L                    # two key buffers at least
                assert w >= prev_l
                prev_l = w
            assert prev_l >= prev_b
            prev_b = prev_l
        assert lib.ltr_sort_workspace_bytes(op, 0, 5000) >= 0
        assert lib.ltr_sort_workspace_bytes(op, -1, 5000) == 0
        assert lib.ltr_sort_workspace_bytes(op, 1, 0) == 0
        assert lib.ltr_sort_workspace_bytes(op, 1, lib.ltr_max_sort_list_len() + 1) == 0
    assert lib.ltr_sort_workspace_bytes(3, 1, 5000) == 0

    def a(x):
        return (x + 255) // 256 * 256
    for op, B, L in ((0, 3, 5000), (1, 16, 100000), (2, 1, 1 << 22)):
        want = a(16 * B * L) + a(4 * L) + (8 * B * ((L + 4095) // 4096) if op else 0)
        assert lib.ltr_sort_workspace_bytes(op, B, L) == want      # the formula of the header
    # about 16-32 B per document
    assert lib.ltr_sort_workspace_bytes(1, 1024, 5000) < 32 * 1024 * 5000


@pytest.mark.parametrize("B", [1, 24])
def test_workspace_formula_grid(lib, B):
    """The header's byte formula where the tile and chunk counts change (one tile more at 4097, 8193; several at 20000).
    ltr_sort_workspace_bytes states it for every valid L (the callers pass no workspace up to ltr_max_list_len())."""
    def a(x):
        return (x + 255) // 256 * 256
    for op in (0, 1, 2):
        for L in (1, 4096, 4097, 8192, 8193, 20000):
            want = a(16 * B * L) + a(4 * L) + (8 * B * ((L + 4095) // 4096) if op else 0)
            assert lib.ltr_sort_workspace_bytes(op, B, L) == want, (op, L)


@pytest.mark.parametrize("seed", [0, 12345, (1 << 62) - 7])
def test_hash_words_long_is_the_library_word_and_a_permutation(lib, seed):
    from pytorchltr_amd import _ties
    M = 1 << 24
    w = _ties.hash_words_long(seed, M)
    assert w.dtype == np.uint32 and w.shape == (M,)
    rng = np.random.default_rng(seed & 0xFFFF)
    for j in np.concatenate([np.arange(16), rng.integers(0, M, 200), [M - 1]]):
        assert int(w[j]) == lib.ltr_tie_hash_word_long(seed, int(j))
    assert np.unique(w).size == M                                   # distinct for every position
    assert lib.ltr_tie_hash_word_long(seed, 0xFFFFFFFF) not in set(int(x) for x in w[:64])


def test_short_tie_word_unchanged(lib):
    """ltr_tie_hash_word (hash19 << 12 | j) is what the <= 4096 path still uses."""
    def word(seed, j):
        m = 0xFFFFFFFF
        h = ((seed & m) ^ ((j * 0x9E3779B1) & m)) & m
        h ^= seed >> 32 & m
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & m
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & m
        h ^= h >> 16
        return ((h >> 13) << 12) | (j & 0xFFF)
    for seed in (0, 7, (1 << 62) - 1):
        got = [lib.ltr_tie_hash_word(seed, j) for j in range(4096)]
        assert got == [word(seed, j) for j in range(4096)]
        assert len(set(got)) == 4096


def test_python_limits_are_host_logic(monkeypatch):
    """Metrics and rankings take lists past 4096 (up to the sort bound); the losses still stop at 4096."""
    import torch
    from pytorchltr_amd import _C, _prepare
    from pytorchltr_amd.evaluation import arp, ndcg
    from pytorchltr_amd.utils import rank_by_score
    monkeypatch.setattr(_C, "require_device", lambda t, what: None)
    with pytest.raises(ValueError):
        _prepare.prepare(torch.zeros(1, 5000), torch.zeros(1, 5000), torch.tensor([1]))
    s, _, _ = _prepare.prepare(torch.zeros(1, 5000), torch.zeros(1, 5000), torch.tensor([1]), limit_len=False)
    assert s.shape == (1, 5000)
    monkeypatch.setattr(_C, "_max_sort_len", 4500)
    with pytest.raises(ValueError, match="exceeds"):
        ndcg(torch.zeros(1, 5000), torch.zeros(1, 5000), torch.tensor([1]), k=10)
    with pytest.raises(ValueError, match="exceeds"):
        arp(torch.zeros(1, 5000), torch.zeros(1, 5000), torch.tensor([1]))
    with pytest.raises(ValueError, match="exceeds"):
        rank_by_score(torch.zeros(1, 5000), torch.tensor([1]))
