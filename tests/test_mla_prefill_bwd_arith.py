"""The element-wise reference of the packed backward at d 192 / d_v 128 (tests/mla_prefill_bwd_cases.py on
oracle.fa2_bwd_arith.restate), pinned on the CPU: it agrees with fp64 autograd within the bars of tests/test_varlen_gpu.py, the same
arithmetic in fp32 passes its own element-wise bars, and the errors a wrong kernel at two widths would make -- planted into the
reference -- break compare() in every sequence they change."""
import functools

import pytest
import torch

import mla_prefill_bwd_cases as C
from oracle import fa2_bwd_arith as A

KERNELS = ("mfma16", "generic")
MASKS = [(False, None), (True, None), (False, (64, 0)), (True, (-1, 17)), (False, (100, 50))]


@pytest.fixture(autouse=True, scope="module")
def one_thread():
    # matrices of a few hundred rows: a thread pool only contends with itself here (30 times slower at 8 threads than at 1)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def problem(dtype, causal, window):
    Q, K, V, dO = C.data(dtype)
    O, L = C.forward_stored(Q, K, V, C.LQ, C.LK, causal, C.SCALE, window)
    return Q, K, V, O, L, dO


@functools.lru_cache(maxsize=None)
def reference(dtype, causal, window, kernel):
    return C.reference(*problem(dtype, causal, window), C.LQ, C.LK, causal, C.SCALE, window, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", (C.BF16, C.F16))
def test_restatement_agrees_with_fp64_autograd(dtype, kernel):
    for causal, window in C.MASKS:
        Q, K, V, O, L, dO = problem(dtype, causal, window)
        ref = reference(dtype, causal, window, kernel)
        assert sorted(ref) == [1, 2, 3, 4, 5, 6]                         # sequence 0 has no query, sequence 7 no key
        got = C.pack(ref, C.LQ, C.LK, (Q, K, V))
        assert got[0].shape == Q.shape and got[1].shape == K.shape and got[2].shape == V.shape
        missed = C.within_truth(got, C.truth(Q, K, V, dO, C.LQ, C.LK, causal, C.SCALE, window), dtype)
        assert not missed, (kernel, causal, window, missed)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", (C.BF16, C.F16))
def test_the_same_arithmetic_in_fp32_passes_compare(dtype, kernel):
    for causal, window in MASKS:
        ref = reference(dtype, causal, window, kernel)
        low = C.reference(*problem(dtype, causal, window), C.LQ, C.LK, causal, C.SCALE, window, kernel, bars=False, acc=torch.float32)
        for b in ref:
            A.assert_close(low[b][:3], ref[b], (kernel, causal, window, b))


def changed(plant, b, nq, nk, causal, window):
    """does this plant change sequence b at all?"""
    if plant in A.MASK_PLANTS:
        return not torch.equal(A.band(nq, nk, causal, window), A.band(nq, nk, causal, window, plant=plant))
    if plant == "last_tile_dropped":
        keep = A.band(nq, nk, causal, window)
        return bool(keep[:, nk - nk % 64:].any()) or bool(keep[nq - nq % 64:].any())
    if plant == "rows_32_exchanged":
        return nk >= 64
    if plant in ("v_at_k_stride", "dv_at_stride_d"):
        return nk > 1                                                    # (row 0 starts where it should)
    return True


@pytest.mark.parametrize("plant", C.PLANTS)
@pytest.mark.parametrize("dtype", (C.BF16, C.F16))
def test_planted_errors_break_compare_in_every_sequence_they_change(dtype, plant):
    hit = 0
    for causal, window in ((False, None), (True, (100, 50))):
        if plant in ("right_plus_one", "left_minus_one") and window is None and not (causal and plant == "right_plus_one"):
            continue                                                     # (an unbounded side has no edge to move)
        args = problem(dtype, causal, window)
        ref = reference(dtype, causal, window, "mfma16")
        bad = C.reference(*args, C.LQ, C.LK, causal, C.SCALE, window, "mfma16", plant=plant, bars=False)
        for b, _, nq, _, nk in C.per_sequence(C.LQ, C.LK):
            if b not in ref:
                continue
            ok = all(r[3] for r in A.compare(bad[b][:3], ref[b]))
            if changed(plant, b, nq, nk, causal, window) and any(not torch.equal(x, y) for x, y in zip(bad[b][:3], ref[b][:3])):
                assert not ok, (plant, causal, window, b, nq, nk)
                hit += 1
            elif not changed(plant, b, nq, nk, causal, window):
                assert ok, (plant, causal, window, b)
    assert hit >= 3, (plant, hit)


@pytest.mark.parametrize("h_kv", (2, 1))
def test_a_wrong_gqa_head_map_misses_the_fp64_group_sum(h_kv):
    # query head h reads KV head h // g; a kernel mapping it h % H_kv sums other heads into dK / dV
    Q, K, V, dO = C.data(C.BF16, h_kv)
    right = C.truth(Q, K, V, dO, C.LQ, C.LK, True, C.SCALE, None)
    assert right[1].shape == K.shape and right[2].shape == V.shape
    wrong = C.truth(Q, K, V, dO, C.LQ, C.LK, True, C.SCALE, None, head_of=[h % h_kv for h in range(C.H)])
    if h_kv == 1:
        assert not C.within_truth(wrong, right, C.BF16)                  # one KV head: both maps are the same map
    else:
        assert C.within_truth(wrong, right, C.BF16)
    assert not C.within_truth(tuple(t.to(C.BF16) for t in right), right, C.BF16)
