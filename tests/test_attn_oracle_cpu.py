"""The attention oracle's bounds, proven on the CPU: the rounding model
stays under them and every mutant of the float64 reference stays well over.

test_gpu_attention_oracle.py holds the HIP kernels to attn_oracle.BOUND.
This file shows, without a GPU, that those bounds are both reachable and
sharp on the very inputs the GPU tests use:

  1. emulate (fp32, rounded to bf16 only where attention.hip rounds) against
     ref64 gives nerr <= BOUND[kind] for all five outputs of every case;
  2. every mutant in attn_oracle.MUTANTS, on every case where it changes
     the math, gives nerr >= TEETH * BOUND[kind] = 3 * BOUND[kind] on the
     outputs it corrupts.

How the bounds were set: FLOOR[kind] is the rounding model's worst nerr over
the 44 grid cases and the 2 spiked-K cases; BOUND = 3 * FLOOR. The factor 3
covers what the model leaves out (__expf, MFMA summation order, the atomic
order of dQ). test_floor_is_what_the_bounds_were_set_from re-measures FLOOR.

Measured (B=2, H=3, GAIN=2, SPIKE=2, SHIFT=12):

  kind   floor     worst case             bound = 3 * floor
  o      2.51e-2   S257 D128 full         7.56e-2
  lse    1.50e-3   S127 D128 causal       4.50e-3
  dq     1.172e-1  S200 D128 full         3.52e-1
  dk     9.87e-2   S191 D128 causal       2.96e-1
  dv     3.59e-2   S127 D128 full         1.08e-1

Smallest nerr of each mutant over the cases it applies to, and that nerr
over the bound (3 is required):

  drop_ragged_tail_keys        o   3.00    39.7  (S1 D64 full)
  padded_keys_unmasked         o   3.00    39.7  (S1 D64 full)
  causal_sees_one_future_key   o   4.63    61.2  (S17 D64 causal)
  causal_hides_own_key         o   3.11    41.1  (S1 D128 causal)
  scale_of_other_head_size     o   0.824   10.9  (S17 D128 causal)
  di_omitted                   dq  2.76     7.9  (S1 D128 causal)
                               dk  2.94     9.9  (S1 D128 causal)
  dq_misses_last_kv_tile       dq  8.70    24.7  (S63 D64 causal)
  dkdv_miss_last_q_tile        dk  6.43    21.7  (S17 D128 full)
                               dv  2.80    25.9  (S1 D64 full)
  dkdv_miss_last_q_row         dk  3.83    12.9  (S127 D64 causal)
                               dv  2.80    25.9  (S1 D64 full)

Cases a mutant is skipped on, because it is a mathematical no-op there:
  the two ragged-tail mutants at S % 64 == 0 (there is no tail), and the
    padded-keys one under causal masking (key >= S > row is masked anyway);
  the causal mutants on the non-causal cases;
  causal_sees_one_future_key, scale_of_other_head_size and
    dq_misses_last_kv_tile at S=1 (no future key; a softmax over one key is
    1 at any scale; dq is zero);
  the dk half of the two dkdv mutants at S=1 (dk is zero with or without
    the row; their dv half is checked there).

The spiked-K cases multiply one K row of the last tile by 8 at S=200 under
causal masking only: without the mask that one key takes over a few whole
rows, the model's own dq floor there is 0.45, and using it would triple the
dq bound for every other case.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as A  # noqa: E402

ALL_CASES = A.CASES + A.KSPIKE_CASES


def _id(case):
    return A.case_id(case[:3]) + ("-kspike" if len(case) > 3 else "")


def test_bounds_are_three_times_the_floor():
    assert A.FACTOR == 3.0 and A.TEETH == 3.0
    assert A.BOUND == {k: 3.0 * f for k, f in A.FLOOR.items()}
    assert len(A.CASES) == 44


@pytest.mark.parametrize("case", ALL_CASES, ids=_id)
def test_rounding_model_within_bounds(case):
    c = A.get_case(*case)
    print(_id(case), {k: f"{e:.3e}" for k, e in c.model.items()})
    for kind in A.KINDS:
        assert c.model[kind] <= A.BOUND[kind], (kind, c.model[kind])


def test_floor_is_what_the_bounds_were_set_from():
    """FLOOR is the model's worst nerr, not a number picked in advance: the
    re-measured worst must not exceed it and must come within 10% of it."""
    worst = {k: max(A.get_case(*c).model[k] for c in ALL_CASES)
             for k in A.KINDS}
    print({k: f"{w:.4e}" for k, w in worst.items()})
    for k in A.KINDS:
        assert 0.9 * A.FLOOR[k] <= worst[k] <= A.FLOOR[k], (k, worst[k])


def test_degenerate_single_key_reference():
    for D in A.D_GRID:
        for causal in (False, True):
            c = A.get_case(1, D, causal)
            assert torch.equal(c.ref["o"], c.v.double())
            assert torch.equal(c.ref["dv"], c.do.double())
            assert c.ref["dq"].abs().max() == 0
            assert c.ref["dk"].abs().max() == 0


def test_reference_matches_autograd():
    """the explicit float64 backward is the gradient of the float64
    forward"""
    c = A.get_case(129, 64, True)
    q, k, v = (t.double().requires_grad_() for t in (c.q, c.k, c.v))
    s = q @ k.transpose(-1, -2) * 64 ** -0.5
    s = s.masked_fill(torch.ones(129, 129, dtype=torch.bool).triu(1),
                      float("-inf"))
    o = torch.softmax(s, -1) @ v
    o.backward(c.do.double())
    for got, kind in ((o, "o"), (q.grad, "dq"), (k.grad, "dk"),
                      (v.grad, "dv")):
        assert A.nerr(got, c.ref[kind]) < 1e-12, kind


@pytest.mark.parametrize("name", list(A.MUTANTS))
def test_mutant_is_caught(name):
    cases = A.mutant_cases(name)
    assert cases
    lo = {}
    for case in cases:
        errs = A.mutant_errors(name, case)
        assert errs, (name, case)
        for kind, e in errs.items():
            assert e >= A.TEETH * A.BOUND[kind], \
                (name, A.case_id(case), kind, e, A.TEETH * A.BOUND[kind])
            if kind not in lo or e < lo[kind][0]:
                lo[kind] = (e, A.case_id(case))
    print(name, {k: (f"nerr {e:.3e}", f"{e / A.BOUND[k]:.1f} x bound", cid)
                 for k, (e, cid) in lo.items()})


def _same(a, b):
    # float64 round-off only (a padded matmul sums in another order)
    return (a - b).abs().max().item() <= 1e-12 * (1.0 + b.abs().max().item())


def test_mutant_skip_list_is_only_noops():
    """a case a mutant is skipped on must be one where it changes nothing"""
    for name, (switches, outs, applies, skip_s) in A.MUTANTS.items():
        for case in A.CASES:
            if applies(*case) and case[0] not in skip_s:
                continue
            c = A.get_case(*case)
            got = A.attn64(c.q, c.k, c.v, c.do, c.causal, **switches(*case))
            for kind in outs:
                assert _same(got[kind], c.ref[kind]), (name, case, kind)
    for (name, S), kinds in A.NOOP_OUTPUTS.items():
        for case in (cs for cs in A.CASES if cs[0] == S):
            c = A.get_case(*case)
            got = A.attn64(c.q, c.k, c.v, c.do, c.causal,
                           **A.MUTANTS[name][0](*case))
            for kind in kinds:
                assert _same(got[kind], c.ref[kind]), (name, case, kind)
