"""The 3x3 convolution case table of tests/conv3x3_cases.py on the CPU: the classifier's constants are the ones in the kernel source,
the table reaches every route the kernels branch on, and every expectation of the exact tier lies in the range where float32 sums and
bf16 stores are exact (which is what lets tests/test_gpu_conv3x3_routes.py assert torch.equal)."""
import pytest
import torch

import conv3x3_cases as C

BF16_EXACT = 256.0        # every integer (and every quarter of an integer) up to 256 has at most 8 significant bits
F32_EXACT = float(2 ** 24)


def test_classifier_constants_are_the_ones_in_the_source():
    texts = {}
    for fname, line, snippet in C.SOURCE_CONSTANTS:
        text = texts.setdefault(fname, C.squeeze_ws(C.source_text(fname)))
        assert C.squeeze_ws(snippet) in text, f"{fname} (was line {line}) no longer contains `{snippet}`: update conv3x3_cases.py"
    src = C.source_text("conv3x3.hip")
    assert f"#define C3_TW {C.TW}" in src and f"#define C3F_TH {C.TH_SHORT}" in src and f"#define C3W_TH {C.WG_TH}" in src
    assert f"H >= {C.TALL_MIN_H} " in src and f"tall ? {C.TH_TALL} : C3F_TH" in src
    assert src.count(f"tiles < {C.MAX_WG} ? tiles : {C.MAX_WG}") == 2
    assert f"Cin <= {C.F32_SMALL_CR})" in src and f"Cin <= {C.BF16_SMALL_CR})" in src
    band = C.source_text("conv3x3_wgrad.hip")
    assert f"#define C3V_TH {C.BAND_TH}" in band and f"#define C3V_TW {C.BAND_TW}" in band
    assert f"(Cin % {C.BAND_C}) == 0 && (Cout % {C.BAND_C}) == 0" in band


def test_classifier_on_hand_worked_shapes():
    r = C.conv_route("bf16", 75, 33, 17, 8, 8)
    assert (r["th"], r["tiles"], r["grid"], r["owners"], r["ck"], r["nck"], r["noc"], r["store"]) == (32, 300, 256, (1, 2), 32, 1, 1, "4")
    r = C.conv_route("bf16", 75, 33, 17, 8, 8, tile32=False)
    assert (r["th"], r["tiles"], r["owners"]) == (16, 450, (1, 2))
    r = C.conv_route("f32", 2, 33, 17, 130, 72)
    assert (r["th"], r["fast"], r["ck"], r["nck"], r["chunk_partial"], r["mb"], r["noc"], r["last_nmb"], r["store"]) == \
        (16, False, 32, 5, True, 5, 2, 1, "4")
    r = C.conv_route("bf16", 1, 65, 33, 96, 192)
    assert (r["th"], r["tiles"], r["fast"], r["ck"], r["nck"], r["chunk_partial"], r["noc"], r["last_nmb"], r["store"]) == \
        (32, 9, True, 64, 2, True, 3, 4, "16")
    assert C.conv_route("bf16", 1, 31, 16, 64, 64)["th"] == 16 and C.conv_route("f32", 1, 64, 16, 64, 64)["th"] == 16
    assert C.conv_route("bf16", 1, 8, 8, 3, 6)["store"] == "scalar" and C.conv_route("bf16", 1, 8, 8, 8, 20)["store4_partial_group"]
    w = C.wgrad_route("bf16", 100, 24, 32, 64, 64)
    assert (w["kernel"], w["tiles"], w["nwg"], w["tpw"], w["idle"]) == ("band", 300, 256, 2, 106)
    assert C.wgrad_route("bf16", 100, 24, 32, 64, 64, scalar_frags=True)["kernel"] == "generic"
    assert C.wgrad_route("f32", 100, 24, 32, 64, 64)["kernel"] == "generic" and C.wgrad_route("bf16", 1, 8, 32, 64, 72)["kernel"] == "generic"
    w = C.wgrad_route("f32", 75, 33, 17, 8, 8)
    assert (w["tiles"], w["nwg"], w["tpw"], w["busy"], w["idle"]) == (450, 256, 2, 225, 31)
    w = C.wgrad_route("bf16", 2, 33, 17, 130, 72)
    assert (w["slices"], w["slice_partial"], w["chunks"], w["chunk_partial"], w["fast_dy"], w["fast_halo"]) == (2, True, 3, True, True, False)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_conv_table_reaches_every_route_for_every_operation(dtype):
    assert 20 <= len(C.CONV_CASES) <= 30 and len({c.name for c in C.CONV_CASES}) == len(C.CONV_CASES)
    for op in C.CONV_OPS:
        reached = set()
        for c in C.CONV_CASES:
            if op in c.ops:
                reached |= C.conv_features(C.conv_route(dtype, c.B, c.H, c.W, c.Cr, c.Cp), c.H, c.W)
        missing = C.CONV_REQUIRED[dtype] - reached
        assert not missing, f"{dtype} {op}: the case table does not reach {sorted(missing)}"
    # the 16-row tile under bf16's persistent loop, and both tile heights over one tall image through the hook
    tall = [c for c in C.CONV_CASES if c.H >= C.TALL_MIN_H]
    assert all(C.conv_route("bf16", c.B, c.H, c.W, c.Cr, c.Cp, tile32=False)["th"] == 16 for c in tall) and len(tall) >= 8
    # the ragged Cp values of the 4-wide and scalar store routes and of partial block groups, and channel counts on both sides of each kernel split
    assert {12, 20, 3, 6, 72, 80} <= {c.Cp for c in C.CONV_CASES}
    assert {16, 17, 32, 33} <= {c.Cr for c in C.CONV_CASES}


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_wgrad_table_reaches_every_route(dtype):
    assert len({c.name for c in C.WGRAD_CASES}) == len(C.WGRAD_CASES) and 40 <= len(C.CONV_CASES) + len(C.WGRAD_CASES) + len(C.TOL_SHAPES) <= 60
    reached = set()
    for c in C.WGRAD_CASES:
        reached |= C.wgrad_features(dtype, c)
    missing = C.WGRAD_REQUIRED[dtype] - reached
    assert not missing, f"{dtype}: the weight-gradient table does not reach {sorted(missing)}"
    assert C.WGRAD_MASKS == ("none", "relu")


def test_tolerance_shapes_are_one_vector_route_and_one_scalar_ragged_route():
    (b, h, w, cin, cout), (b2, h2, w2, cin2, cout2) = C.TOL_SHAPES
    for dtype in C.DTYPES:
        for cr, cp in ((cin, cout), (cout, cin)):
            r = C.conv_route(dtype, b, h, w, cr, cp)
            assert r["fast"] and r["store"] == "16" and h >= 32
        for cr, cp in ((cin2, cout2), (cout2, cin2)):
            r = C.conv_route(dtype, b2, h2, w2, cr, cp)
            assert not r["fast"] and r["store"] == "scalar" and r["rows_partial"] and r["w_ragged"]


def test_no_tensor_of_a_case_is_larger_than_20_mb():
    """(float32 bytes; the band-persistence case 100 x 24 x 32 x 64 is the largest: 19.7 MB per tensor, half of that in bf16)"""
    for c in C.CONV_CASES:
        assert 4 * c.B * c.H * c.W * max(c.Cr, c.Cp) <= 20e6, c.name
    for c in C.WGRAD_CASES:
        assert 4 * c.B * c.H * c.W * max(c.Cin, c.Cout) <= 20e6, c.name


@pytest.mark.parametrize("case", C.CONV_CASES, ids=lambda c: c.name)
def test_conv_exact_expectations_are_exactly_representable(case):
    inputs, expected = C.conv_exact(case)
    assert set(expected) == set(C.CONV_EXPECTED_OPS) and {C.CONV_EXPECTED_OPS[k] for k in expected} == set(case.ops) - {"epi1"}
    m = case.xmax
    assert inputs["x"].abs().max() <= m and inputs["x"].shape == (case.B, case.H, case.W, case.Cr)
    for k in ("w_fwd", "w_bwd"):
        assert set(inputs[k].unique().tolist()) == {-1.0, 0.0, 1.0}
        assert (inputs[k] != 0).float().mean() > 0.5                      # dense: no tap or channel is systematically silent
    # the largest partial sum any summation order can form: 9 taps x Cr channels of |x| <= m, |w| <= 1, then bias and add
    assert 9 * case.Cr * m + 8 + 16 < F32_EXACT
    assert inputs["bias"].abs().max() <= 8 and inputs["add"].abs().max() <= 16 and inputs["sub_from"].abs().max() <= 16
    assert set(inputs["out_y_sig"].unique().tolist()) <= {0.0, 0.5, 1.0}
    for k in ("y_relu_mask", "out_y_relu"):
        assert inputs[k].min() == 0 and inputs[k].max() <= 2
    for name, t in expected.items():
        top = float(t.abs().max())
        print(f"{case.name} {name}: max |v| = {top}")
        # every activation is stored as bf16 in the bf16 runs (and the float32 runs use the same numbers)
        assert top <= BF16_EXACT, f"{case.name} {name}: {top} is not safely exact in bf16; shrink the case's xmax"
        assert torch.equal(t, t.to(torch.bfloat16).float()), f"{case.name} {name} does not survive a bf16 store"
        scale = 4.0 if name == "dx_out_sig" else 1.0
        assert torch.equal(t * scale, (t * scale).round()), f"{case.name} {name} is not integral"
    # what enters the second output as the rounded first output is the first output
    assert torch.equal(expected["out2_both"], inputs["sub_from"] - expected["dx_add"])
    # the unmasked float32 accumulations behind the stored values (before add / mask) are bounded by the plain ones
    assert float(expected["dx_plain"].abs().max()) <= BF16_EXACT and float(expected["y_none"].abs().max()) <= BF16_EXACT


@pytest.mark.parametrize("case", C.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_exact_expectations_are_exactly_representable(case):
    inputs, expected = C.wgrad_exact(case)
    assert set(expected) == {"dw_none", "db_none", "dw_relu", "db_relu"}
    assert inputs["x"].abs().max() <= case.xmax and inputs["dy"].abs().max() <= case.xmax
    # the largest partial sum any summation order can form is bounded by the sum of magnitudes: xmax^2 (xmax for db) per pixel
    assert case.xmax ** 2 * case.B * case.H * case.W < F32_EXACT
    for name, t in expected.items():
        top = float(t.abs().max())
        print(f"{case.name} {name}: max |v| = {top}")
        assert top <= F32_EXACT and torch.equal(t, t.round())
        assert t.shape == ((case.Cout, case.Cin, 3, 3) if name.startswith("dw") else (case.Cout,))
    if case.B * case.H * case.W >= 64:
        assert not torch.equal(expected["dw_none"], expected["dw_relu"])     # the mask matters
