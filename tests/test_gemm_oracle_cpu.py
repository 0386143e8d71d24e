"""The GEMM oracle checked against itself on the CPU: the layer-1
conditions hold on every case, an honest fp32 computation passes both
layers, and every wrong variant fails them (see gemm_oracle.py). No GPU and
no extension; prints the figures docs/KERNELS.md quotes."""

import pytest
import torch

import gemm_oracle as go

ENTRIES = ("gemm", "gemm_skinny", "gemm_nt", "gemm_tn", "bmm")


def _cases(layer, entry):
    return [c for c in go.ALL_CASES if layer in c.layers and c.entry == entry]


def test_case_tables_cover_the_routes():
    ids = {c.id for c in go.ALL_CASES}
    assert len(ids) == len(go.ALL_CASES)
    sk = [c for c in go.CASES if c.entry == "gemm_skinny" and 1 in c.layers]
    for dt in (go.F32, go.BF16):
        assert {c.M for c in sk if c.dtype == dt} >= set(go.SKINNY_M)
        assert {c.N % 64 for c in sk if c.dtype == dt} >= {0, 1, 2, 63}
        assert {c.N for c in sk if c.dtype == dt} >= {1, 2}
    # layer 2 stays where the worst-case bound keeps teeth
    assert all(c.R <= 1100 for c in go.ALL_CASES if 2 in c.layers)
    # the weight of a skinny case stays below about 25M elements
    assert all(c.K * c.N < 25e6 for c in sk)
    assert len(go.GEMM16_CASES) == 4
    assert all(not c.env32 for c in go.GEMM16_CASES)


@pytest.mark.parametrize("entry", ENTRIES)
def test_layer1_conditions_honest_model_and_variants(entry):
    cases = _cases(1, entry)
    assert cases
    seen = set()
    for c in cases:
        smax, nonzero, frac = go.exact_conditions(c)
        print(f"{c.id}: max S {smax:.0f}  non-zero {nonzero}  "
              f"|ref| <= 256: {100 * frac:.2f}%")
        assert smax < 2 ** 24, c
        assert nonzero, c
        if c.out_dtype == go.BF16:
            assert frac >= 0.99, (c, frac)
        for ep in c.eps:
            want = go.exact_ref(c, ep).to(c.out_dtype)
            assert go.check_exact(go.honest_exact(c, ep), c, ep) == 0.0, \
                (c, ep)
            for name, applies in go.VARIANTS1.items():
                if not applies(c, ep):
                    continue
                seen.add(name)
                wrong = go.exact_ref(c, ep, name).to(c.out_dtype)
                assert not torch.equal(wrong, want), (c, ep, name)
                assert go.check_exact(wrong, c, ep) > 0.0
    print(f"{entry}: variants exercised: {sorted(seen)}")
    want_seen = set(go.VARIANTS1) - {"b_untransposed"}
    if not any(c.has_ep for c in cases):
        want_seen -= {"bias_by_row", "resid_before_act", "resid_stride"}
    if entry == "gemm_nt":
        want_seen.add("b_untransposed")
    assert seen >= want_seen, want_seen - seen


def test_activation_error_is_what_the_bound_uses():
    a = go.measure_a_act()
    print(f"A measured {a:.3e}; oracle holds A_ACT_MEASURED "
          f"{go.A_ACT_MEASURED:.3e} x factor {go.A_ACT_FACTOR} = "
          f"{go.A_ACT:.3e}")
    # the host's own tanh may differ a little from the one it was measured
    # with; the factor is there for more than that
    assert 0.75 * go.A_ACT_MEASURED <= a <= 1.25 * go.A_ACT_MEASURED


def _acc_floor():
    """largest err / (sqrt(R) u S) of the honest fp32 model over the
    fp32-output layer-2 cases"""
    worst = 0.0
    for c in go.ALL_CASES:
        if 2 in c.layers and c.out_dtype == go.F32:
            inp = go.inputs2(c)
            A = go.ln64(inp.A, inp.gamma, inp.beta) if c.ln else inp.A
            S = A.abs() @ inp.B.abs()
            if c.has_ep:
                S = S + inp.bias.abs()
            err = (go.honest_model(c).double() - go.ref2(c).out).abs()
            worst = max(worst, (err / (c.R ** 0.5 * go.U * S)).max().item())
    return worst


def test_accumulation_floor_is_what_the_bound_uses():
    f = _acc_floor()
    print(f"honest fp32 model: worst err / (sqrt(R) u S) = {f:.3f}; oracle "
          f"holds ACC_FLOOR {go.ACC_FLOOR} x factor {go.ACC_FACTOR}")
    # the host BLAS's summation order moves this a little
    assert 0.5 * go.ACC_FLOOR <= f <= go.ACC_FLOOR


def test_layer2_bound_is_never_wider_than_the_untightened_form():
    for c in go.ALL_CASES:
        if 2 in c.layers:
            r = go.ref2(c)
            assert (r.bound <= r.bound_issue).all(), c


def test_layer2_honest_model_within_bound_and_variants_far_outside():
    worst_honest = {}
    nearest = {}
    nearest_issue = {}
    for c in go.ALL_CASES:
        if 2 not in c.layers:
            continue
        h = go.check_bound(go.honest_model(c), c)
        key = (c.entry + ("+LN" if c.ln else ""), go.dt_name(c.out_dtype))
        worst_honest[key] = max(worst_honest.get(key, 0.0), h)
        line = f"{c.id}: honest {h:.3f}"
        assert h <= 1.0, (c, h)
        for name, applies in go.VARIANTS2.items():
            if not applies(c):
                continue
            d = go.variant2_distance(c, name)
            di = go.variant2_distance(c, name, issue=True)
            line += f" | {name} {d:.2f} (untightened {di:.2f})"
            assert d >= go.TEETH, (c, name, d)
            nearest[name] = min(nearest.get(name, float("inf")), d)
            nearest_issue[name] = min(nearest_issue.get(name, float("inf")),
                                      di)
        print(line)
    print("worst honest err / bound per (entry, output):")
    for k, v in sorted(worst_honest.items()):
        print(f"  {k[0]} {k[1]}: {v:.3f}")
    print("smallest variant distance (bounds), and against the untightened "
          "bound (2 R u S, 1e-4 S_ln, 2^-8 S_ln, 2^-7 |ref|):")
    for k in sorted(nearest):
        print(f"  {k}: {nearest[k]:.2f}   [{nearest_issue[k]:.2f}]")
    assert set(nearest) == set(go.VARIANTS2)
    # the module's docstring quotes these; keep it honest
    for name, quoted in go.MEASURED_TEETH.items():
        assert abs(nearest[name] - quoted) <= 0.03 * quoted, \
            (name, nearest[name], quoted)


def test_guard_band_layout():
    t = torch.arange(12.0).reshape(3, 4)
    for ua in (False, True):
        v = go.guarded(t, go.F32, "cpu", ua)
        assert v.is_contiguous() and torch.equal(v, t)
        off = v.storage_offset()
        assert off == go.GUARD + int(ua)
        assert (off * 4 % 16 == 0) != ua and (off * 2 % 16 == 0) != ua
        whole = torch.as_strided(v, (v.untyped_storage().nbytes() // 4,),
                                 (1,), 0)
        assert torch.isnan(whole[:off]).all()
        assert torch.isnan(whole[off + 12:]).all()
        assert whole.numel() - off - 12 >= go.GUARD
