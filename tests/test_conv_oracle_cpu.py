"""The conv oracle checked against itself on the CPU: the layer-1 conditions
hold on every case, torch's own convolution (float64 and fp32) equals the
gathered reference on layer 1 and stays within the bound on layer 2, every
wrong variant fails, and the case table reaches every route (see
conv_oracle.py). No GPU and no extension; prints the figures
docs/KERNELS.md quotes."""

import pytest
import torch

import conv_oracle as co
import gemm_oracle as go


def test_oracle_reuses_the_gemm_constants():
    assert co.ACC == go.ACC_FACTOR * go.ACC_FLOOR
    assert co.TEETH == go.TEETH == 3.0 and co.GUARD == go.GUARD


def test_case_table_has_the_shapes_the_suite_never_had():
    cs = co.CASES
    assert any(c.H != c.W for c in cs) and any(c.OH != c.OW for c in cs)
    assert any(c.KH != c.KW for c in cs) and any(c.SH != c.SW for c in cs)
    assert any(c.PH != c.PW for c in cs)
    assert any(c.KH == 3 and c.PH == 0 and c.PW == 0 for c in cs)
    assert any(c.unaligned and c.dtype == dt for c in cs
               for dt in (co.BF16, co.F32))
    assert sum(c.nhwc for c in cs) == 1
    assert any(co.big_y(c) for c in cs)
    l2 = co.cases_for(2)
    assert 8 <= len(l2) <= 14 and all(c.K <= 1152 for c in l2)
    assert {c.dtype for c in l2} == {co.BF16, co.F32}
    assert any(c.H != c.W for c in l2) and any(c.PH != c.PW for c in l2)
    # both tile widths in every direction (wide: no N tail at 128)
    assert any(c.Cout % 128 == 0 for c in l2) and any(c.Cout % 128 for c in l2)
    assert any(c.Cin % 128 == 0 for c in l2) and any(c.Cin % 128 for c in l2)


@pytest.mark.parametrize("c", co.CASES, ids=lambda c: c.id)
def test_layer1_conditions_honest_models_and_variants(c):
    smax, sabs, ssq = co.exact_conditions(c)
    print(f"{c.id}: max S {smax:.0f}  max sum|y| {sabs:.0f}  "
          f"max sum y^2 {ssq:.3g}  some |y| > 256: {co.big_y(c)}")
    for key in c.keys:
        want = co.exact_ref(c, key)
        assert not torch.isnan(want).any()
        # torch's own convolution, float64 cast once and plain fp32
        for dtype in (torch.float64, torch.float32):
            assert co.check_exact(co.honest(c, 1, key, dtype), c, key) == 0.0, \
                (c, key, dtype)
        for name, applies in co.VARIANTS1.items():
            if applies(c, key):
                wrong = co.exact_ref(c, key, name)
                assert wrong.shape == want.shape
                assert not torch.equal(wrong, want), (c, key, name)
                assert co.check_exact(wrong, c, key) > 0.0


def test_layer1_variants_each_apply_to_at_least_two_cases():
    count = {name: sum(any(applies(c, k) for k in c.keys) for c in co.CASES)
             for name, applies in co.VARIANTS1.items()}
    print(count)
    assert all(n >= 2 for n in count.values()), count
    # the statistics variant needs outputs that a bf16 rounding changes
    assert sum(co.big_y(c) and c.dtype == co.BF16 for c in co.CASES) >= 2


def test_exact_conditions_have_room():
    worst = [0.0, 0.0, 0.0]
    for c in co.CASES:
        worst = [max(a, b) for a, b in zip(worst, co.exact_conditions(c))]
    print("max S %.0f, max sum|y| %.0f, max sum y^2 %.4g (limit 2^24 = %d)"
          % (*worst, 2 ** 24))
    assert max(worst) < 2 ** 23


def _acc_floor():
    """largest err / (sqrt(R) u S) of the honest fp32 model over the
    fp32 outputs of the layer-2 cases"""
    worst = 0.0
    for c in co.cases_for(2):
        for key in c.keys:
            if key == "stats" or c.out_dtype(key) != co.F32:
                continue
            r = co.ref2(c, key)
            err = (co.honest(c, 2, key).double() - r.out).abs()
            tail = 2 * co.U * r.out.abs() + 1e-30
            S = (r.bound - tail) / (min(co.ACC * c.R(key) ** 0.5,
                                        2 * c.R(key)) * co.U)
            worst = max(worst,
                        (err / (c.R(key) ** 0.5 * co.U * S)).max().item())
    return worst


def test_accumulation_floor_holds_on_the_conv_summation_shapes():
    f = _acc_floor()
    print(f"honest fp32 conv model: worst err / (sqrt(R) u S) = {f:.3f}; the "
          f"bound uses ACC_FLOOR {go.ACC_FLOOR} x factor {go.ACC_FACTOR}")
    assert f <= go.ACC_FLOOR


def test_layer2_bound_is_never_wider_than_the_plain_form():
    for c in co.cases_for(2):
        for key in c.keys:
            r = co.ref2(c, key)
            assert (r.bound <= r.bound_plain).all(), (c, key)


def test_layer2_honest_model_within_bound_and_variants_far_outside():
    worst_honest, nearest, nearest_plain = {}, {}, {}
    for c in co.cases_for(2):
        line = f"{c.id}:"
        for key in c.keys:
            h = co.check_bound(co.honest(c, 2, key), c, key)
            k2 = (key, go.dt_name(c.out_dtype(key)))
            worst_honest[k2] = max(worst_honest.get(k2, 0.0), h)
            assert h <= 1.0, (c, key, h)
            line += f" {key} {h:.3f}"
            for name, applies in co.VARIANTS2.items():
                if not applies(c, key):
                    continue
                d = co.variant2_distance(c, key, name)
                dp = co.variant2_distance(c, key, name, plain=True)
                line += f" [{name} {d:.2f}, plain {dp:.2f}]"
                assert d >= co.TEETH, (c, key, name, d)
                nearest[name] = min(nearest.get(name, float("inf")), d)
                nearest_plain[name] = min(
                    nearest_plain.get(name, float("inf")), dp)
        print(line)
    print("worst honest err / bound per (output, dtype):")
    for k, v in sorted(worst_honest.items()):
        print(f"  {k[0]} {k[1]}: {v:.3f}")
    print("smallest variant distance (bounds), and against the plain bound "
          "(2 R u S + 2^-7 |ref|):")
    for k in sorted(nearest):
        print(f"  {k}: {nearest[k]:.2f}   [{nearest_plain[k]:.2f}]")
    assert set(nearest) == set(co.VARIANTS2)
    for name, quoted in co.MEASURED_TEETH.items():
        assert abs(nearest[name] - quoted) <= 0.03 * quoted, \
            (name, nearest[name], quoted)


# every name conv2d_fwd_route, conv2d_dgrad_route and conv2d_wgrad_route can
# return (conv2d.hip); a new route without a case fails this test
ROUTE_NAMES = {
    "fwd": ["k_conv_fwd_sb_wide", "k_conv_fwd_db_wide", "k_conv_fwd_sb",
            "k_conv_fwd_db", "k_conv_fwd<pow2, glds>", "k_conv_fwd<pow2>",
            "k_conv_fwd"],
    "dgrad": ["k_conv_dgrad_sb_wide<S2>", "k_conv_dgrad_sb_wide<S1>",
              "k_conv_dgrad_sb_wide", "k_conv_dgrad_db_wide<S2>",
              "k_conv_dgrad_db_wide<S1>", "k_conv_dgrad_db_wide",
              "k_conv_dgrad_db<S2>", "k_conv_dgrad_db<S1>", "k_conv_dgrad_db",
              "k_conv_dgrad<pow2, glds, S2>", "k_conv_dgrad<pow2, glds, S1>",
              "k_conv_dgrad<pow2, glds>", "k_conv_dgrad<pow2>",
              "k_conv_dgrad"],
    "wgrad": ["k_conv_wgrad_tr_wide<db>", "k_conv_wgrad_tr_wide<sb>",
              "k_conv_wgrad_tr", "k_conv_wgrad_vec", "k_conv_wgrad<pow2>",
              "k_conv_wgrad"],
}


def test_every_route_is_the_expected_route_of_some_case():
    assert set(ROUTE_NAMES["fwd"]) == set(co.FWD_ROUTES)
    assert set(ROUTE_NAMES["dgrad"]) == set(co.DGRAD_ROUTES)
    assert set(ROUTE_NAMES["wgrad"]) == set(co.WGRAD_ROUTES)
    seen = {"fwd": set(), "fwd_stats": set(), "dgrad": set(), "wgrad": set()}
    zs = set()
    for child in co.CHILDREN:
        for c in co.CASES:
            r = co.expected_routes(c, child)
            if "y" in c.keys:
                seen["fwd"].add(r["fwd"])
                seen["fwd_stats"].add(r["fwd_stats"])
            if "dx" in c.keys:
                seen["dgrad"].add(r["dgrad"])
            seen["wgrad"].add(r["wgrad"][0])
            zs.add(r["wgrad"][1])
    for k, names in seen.items():
        want = set(ROUTE_NAMES["fwd" if k == "fwd_stats" else k])
        assert names == want, (k, want ^ names)
    assert {1, 4, 29} <= zs, zs


def test_expected_routes_of_the_cases_the_parity_gate_moved():
    """stride 2 with KW > 4 stays off the parity (S2) kernels in every
    child; KW <= 4 with a tall kernel stays on them"""
    for c in co.CASES:
        if c.SH == 2 and c.SW == 2 and not c.unaligned \
                and c.dtype == co.BF16 and c.label != "nonpow2":
            for child in co.CHILDREN:
                r = co.dgrad_route(c, child)
                assert ("S2" in r) == (c.KW <= 4), (c, child, r)
    by = {c.label: c for c in co.CASES}
    assert co.dgrad_route(by["k5x5_s2"], "default") == "k_conv_dgrad_db"
    assert co.dgrad_route(by["k7x7_s2"], "default") == "k_conv_dgrad_db"
    assert co.dgrad_route(by["k5x5_s2_wide"], "wide_db") == \
        "k_conv_dgrad_db_wide"
    assert co.dgrad_route(by["k7x7_s2_wide"], "default") == \
        "k_conv_dgrad<pow2, glds>"
    assert co.dgrad_route(by["k5x5_s2"], "nodb") == "k_conv_dgrad<pow2, glds>"
    assert co.dgrad_route(by["k5x3_s2_p2x1"], "default") == \
        "k_conv_dgrad_db<S2>"
    assert co.dgrad_route(by["k4x4_s2"], "default") == "k_conv_dgrad_db<S2>"


def test_guarded_operands_are_views_into_nan_buffers():
    c = co.BY_ID[[i for i in co.BY_ID if i.endswith("-unal")][0]]
    for t in co.device_operands(c, 1, "cpu"):
        assert t.is_contiguous() and t.storage_offset() == co.GUARD + 1
        assert not torch.isnan(t).any()
