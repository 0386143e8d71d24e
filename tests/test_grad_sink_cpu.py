"""Host-side bookkeeping of the gradient sinks (no GPU): the registry's
overwrite-then-accumulate marks and the zeroing plan GraphedTrainStep derives
from the set of parameters the sinks wrote."""

import pytest
import torch

from tnn_amd.ops.functional import GradSinks
from tnn_amd.utils.graphstep import unwritten_runs


def _params(*shapes):
    ps = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    for p in ps:
        p.grad = torch.zeros_like(p)
    return ps


def test_first_write_overwrites_later_ones_accumulate():
    a, b = _params((3, 4), (5,))
    sinks = GradSinks([a, b])
    ka, kb = a.data_ptr(), b.data_ptr()
    assert sinks.get(ka) is a.grad and sinks.get(kb) is b.grad
    assert sinks.claim(ka) is False        # first write of the step
    assert sinks.claim(ka) is True         # the layer applied again
    assert sinks.written == {ka}
    sinks.begin_step()
    assert sinks.written == set()
    assert sinks.claim(ka) is False
    assert sinks.claim(kb) is False


def test_lookup_misses():
    a, = _params((3, 4))
    sinks = GradSinks([a])
    assert sinks.get(None) is None
    assert sinks.get(12345) is None
    # a tensor of another shape or dtype reaching the backward: no sink
    assert sinks.get(a.data_ptr(), torch.zeros(4, 3)) is None
    assert sinks.get(a.data_ptr(), torch.zeros(3, 4).bfloat16()) is None
    assert sinks.get(a.data_ptr(), torch.zeros(3, 4)) is a.grad


def test_register_rejects_unfit_buffers():
    a, = _params((3, 4))
    sinks = GradSinks()
    for bad in (None, torch.zeros(4, 3), torch.zeros(3, 4).bfloat16(),
                torch.zeros(4, 3).t()):
        with pytest.raises(ValueError):
            sinks.register(a, bad)


LAYOUT = [("a", 0, 10), ("b", 10, 20), ("c", 30, 5), ("d", 35, 100),
          ("e", 135, 1), ("f", 136, 0)]


def test_unwritten_runs_joins_neighbours():
    assert unwritten_runs(LAYOUT, set(), merge_gap=0) == [(0, 136)]
    assert unwritten_runs(LAYOUT, set("abcde"), merge_gap=0) == []
    assert unwritten_runs(LAYOUT, {"b", "d"}, merge_gap=0) == \
        [(0, 10), (30, 35), (135, 136)]
    assert unwritten_runs(LAYOUT, {"a"}, merge_gap=0) == [(10, 136)]


def test_unwritten_runs_merges_across_small_gaps_only():
    # gaps: b = 20 elements, d = 100
    assert unwritten_runs(LAYOUT, {"b", "d"}, merge_gap=20) == \
        [(0, 35), (135, 136)]
    assert unwritten_runs(LAYOUT, {"b", "d"}, merge_gap=19) == \
        [(0, 10), (30, 35), (135, 136)]
    assert unwritten_runs(LAYOUT, {"b", "d"}, merge_gap=100) == [(0, 136)]


def test_every_unwritten_element_is_covered():
    g = torch.Generator().manual_seed(0)
    sizes = torch.randint(0, 50, (40,), generator=g).tolist()
    layout, off = [], 0
    for i, n in enumerate(sizes):
        layout.append((i, off, n))
        off += n
    written = set(torch.randperm(40, generator=g)[:25].tolist())
    for gap in (0, 7, 1000):
        covered = torch.zeros(off, dtype=torch.bool)
        runs = unwritten_runs(layout, written, merge_gap=gap)
        for a, b in runs:
            assert 0 <= a < b <= off
            covered[a:b] = True
        assert all(r1[1] < r2[0] for r1, r2 in zip(runs, runs[1:]))
        for key, o, n in layout:
            if key not in written:
                assert covered[o:o + n].all()


def test_two_destination_split_rule():
    """splitk_reduce_can_split, the host arithmetic that decides whether the
    reduce may write [0, n0) and [n0, n) to two places: always on the scalar
    kernel (n % 4 != 0); on the float4 kernels only with the boundary on a
    group of 4 and both destinations aligned to 4 elements."""
    from tnn_amd import _C
    can = _C.ext().splitk_can_split
    base = 1 << 20
    for bf16, el in ((False, 4), (True, 2)):
        assert can(1152 + 128, 1152, base, base + 4 * el * 300, bf16)
        # boundary off a group of 4 while n % 4 == 0
        assert not can(24, 10, base, base + 4 * el * 300, bf16)
        # either destination off 4 elements
        assert not can(1280, 1152, base + el, base + 4 * el * 300, bf16)
        assert not can(1280, 1152, base, base + 4 * el * 300 + 2 * el, bf16)
        # n % 4 != 0: the scalar kernel splits anywhere, at any alignment
        assert can(730, 720, base + el, base + 3 * el, bf16)
        assert can(731, 721, base + el, base + 3 * el, bf16)
    # 8-byte alignment is enough for bf16 groups, not for fp32 ones
    assert can(1280, 1152, base + 8, base + 4096, True)
    assert not can(1280, 1152, base + 8, base + 4096, False)
