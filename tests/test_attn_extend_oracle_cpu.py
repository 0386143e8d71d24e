"""The extend-attention oracle, proven on the CPU.

test_gpu_attn_extend.py holds attn::k_attn_ext to attn_oracle.BOUND["o"]
(7.56e-2) on the launches of attn_extend_oracle.py. This file shows, without
a GPU, on those very launches:

  1. extend64 with every switch off reproduces the reference cut out of the
     attn_oracle cases (the construction is what it says it is);
  2. the rounding model's worst error stays at or below attn_oracle.FLOOR["o"]
     (2.52e-2), so the unchanged bound is reachable;
  3. four wrong float64 variants each land at least TEETH * BOUND away on
     every launch where they change the math;
  4. the torch form behind ops.attention_extend (what every non-HIP route
     runs) meets the same bound, returns exact zeros for rows >= n_new[b],
     and lets no NaN from a dead cache slot through; ops.kv_append_n drops
     overflowing rows and rows of a negative position.

Measured (B=2, H=3, cap=300, 9 launches x D in {64, 128}):

  rounding model, worst     2.37e-2   P299T1-P172T128-D64   (floor 2.52e-2)

  mutant                       smallest nerr   over the bound
  causal_sees_one_future_key   3.22            42.6   (P299T1-P172T128-D64)
  causal_hides_own_key         2.98            39.4   (P63T2-P64T1-D128)
  every_row_uses_row0_pos      2.85            37.8   (P63T2-P64T1-D64)
  drop_ragged_tail_keys        2.98            39.4   (P63T2-P64T1-D128)

The +1 mutant reads the cache as it is: for a live row the causal rule alone
keeps every key below the live length, so a rule that is off by one reaches
the dead slot behind the last live key. With plain random poison that slot
takes a visible share of the softmax only by chance (0.15 on P63T2-P64T1-D64,
two bounds), so the launches move that one key along the row's last query
until it would take half of its softmax, as attn_oracle does with the spiked
rows' own keys.

Skipped as mathematical no-ops: row 0's pos on launch 0 (both rows have
pos = 0) and the dropped tail on launch 1 (both live lengths are 64).
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as A  # noqa: E402
import attn_extend_oracle as X  # noqa: E402

from tnn_amd import ops  # noqa: E402


def test_launch_list_is_the_issues():
    assert X.LAUNCHES == [
        [(0, 1), (0, 17)], [(0, 64), (63, 1)], [(63, 2), (64, 1)],
        [(1, 64), (47, 17)], [(48, 17), (0, 129)], [(100, 100), (191, 9)],
        [(127, 130), (255, 2)], [(120, 8), (5, 3)], [(299, 1), (172, 128)]]
    assert (X.B, X.H, X.CAP) == (2, 3, 300) and X.D_GRID == [64, 128]
    assert A.BOUND["o"] == 3.0 * 2.52e-2


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_rule_reproduces_the_cut_out_reference(case):
    L = X.get_launch(*case)
    o = X.extend64(L.q, L.kc, L.vc, L.pos, L.n_new)
    assert L.error(o) < 1e-12
    assert L.dead_rows_zero(o)


def test_rounding_model_stays_under_the_floor():
    worst = {c: X.get_launch(*c).model for c in X.CASES}
    top = max(worst, key=worst.get)
    print(f"model worst {worst[top]:.3e} at {X.case_id(top)}")
    assert worst[top] <= A.FLOOR["o"]


@pytest.mark.parametrize("name", list(X.MUTANTS))
def test_mutant_is_caught(name):
    applies = X.MUTANTS[name][1]
    cases = [c for c in X.CASES if applies(c[0])]
    skipped = sorted({c[0] for c in X.CASES} - {c[0] for c in cases})
    assert skipped == {"every_row_uses_row0_pos": [0],
                       "drop_ragged_tail_keys": [1]}.get(name, [])
    errs = {c: X.mutant_error(name, c) for c in cases}
    lo = min(errs, key=errs.get)
    print(f"{name}: smallest nerr {errs[lo]:.3e} = "
          f"{errs[lo] / A.BOUND['o']:.1f} x bound at {X.case_id(lo)}")
    for c, e in errs.items():
        assert e >= A.TEETH * A.BOUND["o"], (name, X.case_id(c), e)


def test_mutant_skips_are_noops():
    for name, idx in (("every_row_uses_row0_pos", 0),
                      ("drop_ragged_tail_keys", 1)):
        for D in X.D_GRID:
            assert X.mutant_error(name, (idx, D)) < 1e-12


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_torch_form_within_bound(case):
    L = X.get_launch(*case)
    o = ops.attention_extend(L.q, L.kc, L.vc, L.pos, L.n_new)
    assert o.shape == L.q.shape and o.dtype == torch.bfloat16
    assert o.transpose(1, 2).is_contiguous()
    L.check("torch form " + X.case_id(case), o)
    assert L.dead_rows_zero(o)


def test_torch_form_ignores_nan_in_dead_slots_and_uniform_chunks():
    L = X.get_launch(5, 64)
    o = ops.attention_extend(L.q, L.kc, L.vc, L.pos, L.n_new)
    kn, vn = L.nan_poisoned()
    assert torch.equal(ops.attention_extend(L.q, kn, vn, L.pos, L.n_new), o)
    full = torch.full_like(L.n_new, L.T)
    pos0 = torch.zeros_like(L.pos)
    assert torch.equal(ops.attention_extend(L.q, L.kc, L.vc, pos0, None),
                       ops.attention_extend(L.q, L.kc, L.vc, pos0, full))


def test_torch_form_clamps_positions():
    """pos past the cache: n clamps to 0 and the row comes back zero;
    a chunk that would run past cap is cut at cap"""
    L = X.get_launch(7, 64)
    pos = torch.tensor([X.CAP + 5, X.CAP - 2])
    o = ops.attention_extend(L.q, L.kc, L.vc, pos, None)
    assert bool((o[0] == 0).all()) and bool((o[1, :, 2:] == 0).all())
    want = X.extend64(L.q, L.kc, L.vc, pos, torch.full_like(pos, L.T))
    assert A.nerr(o[1, :, :2], want[1, :, :2]) <= A.BOUND["o"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kv_append_n_torch_form(dtype):
    Bn, Hn, T, D, cap = 4, 2, 5, 8, 40
    g = torch.Generator().manual_seed(3)
    merged = torch.randn(Bn, T, 3 * Hn * D, generator=g).to(dtype)
    _, k, v = (t.view(Bn, T, Hn, D).transpose(1, 2)
               for t in merged.split(Hn * D, dim=-1))
    kc = torch.full((Bn, Hn, cap, D), 7.0, dtype=dtype)
    vc = torch.full((Bn, Hn, cap, D), -7.0, dtype=dtype)
    pos = torch.tensor([37, 0, 17, -1])
    n_new = torch.tensor([5, 0, 3, 5])
    ops.kv_append_n(kc, vc, k, v, pos, n_new)
    wk, wv = torch.full_like(kc, 7.0), torch.full_like(vc, -7.0)
    wk[0, :, 37:40], wv[0, :, 37:40] = k[0, :, :3], v[0, :, :3]
    wk[2, :, 17:20], wv[2, :, 17:20] = k[2, :, :3], v[2, :, :3]
    assert torch.equal(kc, wk) and torch.equal(vc, wv)
    ops.kv_append_n(kc, vc, k, v, torch.tensor([0, 1, 2, 3]), None)
    for b in range(Bn):
        assert torch.equal(kc[b, :, b:b + T], k[b])
        assert torch.equal(vc[b, :, b:b + T], v[b])
