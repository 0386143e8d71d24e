"""The split-KV extend-attention oracle, proven on the CPU.

test_gpu_attn_extend_split.py holds attn::k_attn_ext_split + k_attn_ext_fin
to attn_oracle.BOUND["o"] (7.56e-2) on the launches of
attn_extend_split_oracle.py, at every split count in {1, 2, 3, 4, 8, 16}.
This file shows, without a GPU, on those very launches:

  1. split64 with every switch off reproduces the reference cut out of the
     attn_oracle cases, at every split count (the split rule is the rule);
  2. the rounding model of the split form (attn_oracle.emulate's roundings
     inside each split, then the fp32 combine) stays within a third of the
     bound, the margin the bound was given over its own model;
  3. seven wrong float64 variants each land at least TEETH * BOUND away on
     every (launch, D, split count) where they change the math;
  4. ops.attention_extend's torch form takes kv_splits and ignores it.

Measured (B=2, H=3, cap=640, 7 launches x D in {64, 128} x 6 split counts):

  rounding model, worst     1.91e-2   P127T2-P128T16-D128-NS1   (bound / 3 = 2.52e-2)

  mutant                        smallest nerr   over the bound
  last_nonempty_split_dropped   2.63            34.8   (P63T1-P64T1-D64-NS1)
  combine_without_weights       1.05            13.9   (P63T1-P64T1-D128-NS2)
  boundary_one_tile_late        1.77            23.4   (P624T16-P639T1-D128-NS2)
  boundary_one_tile_early       0.466            6.2   (P100T0-P200T5-D64-NS4)
  every_row_uses_row0_pos       2.85            37.8   (P63T1-P64T1-D64-NS1)
  causal_sees_one_future_key    11.3           148.8   (P63T1-P64T1-D64-NS1)
  causal_hides_own_key          2.85            37.8   (P63T1-P64T1-D64-NS1)

"late" starts every split after the first one tile late, "early" runs every
split but the last one tile into the next.

Skipped as mathematical no-ops (asserted): the three split-boundary mutants
where no live row is shared by two non-empty splits (split count 1
everywhere, and launch 0, whose rows have one tile), and row 0's pos on
launch 0 (both rows have pos = 0).

Skipped by structure, and no no-op: the +1 causal rule on launch 5. As in
attn_extend_oracle, that mutant is caught through the spiked dead key behind
a row's last live key. Launch 5 fills both rows to CAP = 640, so no such
slot exists; the rule there only shows rows 0..14 of the 16-row chunk the
next row's live key, one random key among 626 or more, and lands at 0.98
(D64) and 0.21 (D128) bounds. test_future_key_mutant_at_the_brim prints
those figures and asserts the structural reason.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as A  # noqa: E402
import attn_extend_split_oracle as X  # noqa: E402

from tnn_amd import ops  # noqa: E402


def test_launch_list_is_the_issues():
    assert X.LAUNCHES == [
        [(0, 1), (0, 16)], [(63, 1), (64, 1)], [(127, 2), (128, 16)],
        [(300, 8), (5, 3)], [(191, 9), (255, 2)], [(624, 16), (639, 1)],
        [(100, 0), (200, 5)]]
    assert X.SPLITS == [1, 2, 3, 4, 8, 16]
    assert (X.B, X.H, X.CAP) == (2, 3, 640) and X.D_GRID == [64, 128]
    assert A.BOUND["o"] == 3.0 * 2.52e-2


def test_split_shares():
    """ten tiles over 3 and 4 are uneven, over 16 leave empty splits; a
    one-tile row sits next to a ten-tile row"""
    assert [X.split_tiles(640, 3, s) for s in range(3)] == [
        (0, 4), (4, 8), (8, 10)]
    assert [X.split_tiles(640, 4, s) for s in range(4)] == [
        (0, 3), (3, 6), (6, 9), (9, 10)]
    assert [X.split_tiles(640, 16, s) for s in (9, 10, 15)] == [
        (9, 10), (10, 10), (15, 10)]
    assert [X.split_tiles(8, 4, s) for s in range(4)] == [
        (0, 1), (1, 1), (2, 1), (3, 1)]
    assert X.split_tiles(308, 2, 1) == (3, 5)


@pytest.mark.parametrize("lcase", X.LCASES, ids=X.launch_id)
def test_rule_reproduces_the_cut_out_reference(lcase):
    L = X.get_launch(*lcase)
    for ns in X.SPLITS:
        o = X.split64(L.q, L.kc, L.vc, L.pos, L.n_new, ns)
        assert L.error(o) < 1e-12, ns
        assert L.dead_rows_zero(o)


def test_rounding_model_within_a_third_of_the_bound():
    worst = {c: X.model_error(*c) for c in X.CASES}
    top = max(worst, key=worst.get)
    print(f"split model worst {worst[top]:.3e} at {X.case_id(top)} "
          f"(bound / 3 = {A.BOUND['o'] / 3:.3e})")
    for c, e in worst.items():
        assert e <= A.BOUND["o"] / 3, (X.case_id(c), e)


NOOPS = {
    "combine_without_weights": "one_split",
    "boundary_one_tile_late": "one_split",
    "boundary_one_tile_early": "one_split",
    "every_row_uses_row0_pos": "launch0",
}
# skipped by structure, not a no-op: see test_future_key_mutant_at_the_brim
BRIM = {"causal_sees_one_future_key": "launch5"}


@pytest.mark.parametrize("name", list(X.MUTANTS))
def test_mutant_is_caught(name):
    applies = X.MUTANTS[name][1]
    cases = [c for c in X.CASES if applies(c[0], c[2])]
    skipped = sorted(set(X.CASES) - set(cases))
    want = {"one_split": [c for c in X.CASES if c[2] == 1 or c[0] == 0],
            "launch0": [c for c in X.CASES if c[0] == 0],
            "launch5": [c for c in X.CASES if c[0] == 5],
            None: []}[NOOPS.get(name, BRIM.get(name))]
    assert skipped == sorted(want)
    errs = {c: X.mutant_error(name, c) for c in cases}
    lo = min(errs, key=errs.get)
    print(f"{name}: smallest nerr {errs[lo]:.3e} = "
          f"{errs[lo] / A.BOUND['o']:.1f} x bound at {X.case_id(lo)}")
    for c, e in errs.items():
        assert e >= A.TEETH * A.BOUND["o"], (name, X.case_id(c), e)


def test_mutant_skips_are_noops():
    for name in NOOPS:
        applies = X.MUTANTS[name][1]
        for c in X.CASES:
            if not applies(c[0], c[2]):
                assert X.mutant_error(name, c) < 1e-12, (name, X.case_id(c))


def test_future_key_mutant_at_the_brim():
    """Launch 5 fills both rows to CAP, so there is no dead slot for the +1
    rule to read: all it does there is show rows 0..14 of the 16-row chunk
    the next row's live key, one random key among 626 or more. That changes
    the result (this is no no-op) but only by chance visibly, and the
    launch is left out of the mutant's cases for that structural reason.
    The figures are printed."""
    for D in X.D_GRID:
        e = X.mutant_error("causal_sees_one_future_key", (5, D, 1))
        print(f"+1 at the brim, D{D}: nerr {e:.3e} = "
              f"{e / A.BOUND['o']:.2f} x bound")
        assert e > 1e-6
    assert all(P + T == X.CAP for P, T in X.LAUNCHES[5])
    assert all(any(P + T < X.CAP for P, T in rows if T > 0)
               for i, rows in enumerate(X.LAUNCHES) if i != 5)


def test_torch_form_ignores_kv_splits():
    L = X.get_launch(3, 64)
    o = ops.attention_extend(L.q, L.kc, L.vc, L.pos, L.n_new)
    for ns in (0, 4, 16):
        assert torch.equal(
            ops.attention_extend(L.q, L.kc, L.vc, L.pos, L.n_new,
                                 kv_splits=ns), o)
    L.check("torch form " + X.launch_id((3, 64)), o, 1)
    assert L.dead_rows_zero(o)
