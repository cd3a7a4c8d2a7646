"""The split-mode (FFH_MATH_FP32_SPLIT_BF16X3_ALL) Linear sweep's harness (tests/linear_helpers.py, Case.mode = 3), proved on a CPU, without the kernels.

The "planes" generator has to meet its own conditions for every case of the edge table.  The six-product restatement (NumpySplitLib: the entry
points in numpy, written from include/ff_hip.h) has to pass the checker; every mutant of it -- one product dropped, the third plane dropped, a3
paired with b2, a truncating split -- has to be rejected on "planes", while on "uniform" the mutant without a third plane still holds the
project's bound: that is asserted, as the record of why the family exists.  The oracle library, which sums unsplit fp32 products in this mode,
passes the other distributions and is rejected on "planes".  The image checker has to report swapped planes, a written padding position, a
stale element and an unwritten image under a bf16x3 route.  And the route model at 256 CUs has to reach every token the table names.
"""
import numpy as np
import pytest

import linear_helpers as LH
from linear_helpers import Case, NONE, RELU, SIG, OVERWRITE, ONLY_DW, ONLY_DX, MASK_BY_X, PREMASKED, MATH_SPLIT_ALL, SIX

M3 = dict(mode=MATH_SPLIT_ALL)
EMULATED_WORK = 3e8          # table cases up to this batch * in * out go through the numpy entry points here (the others on the GPU only)


@pytest.fixture(scope="module")
def olib(oracle):
    return oracle.lib()


def _small(cases):
    return [c for c in cases if c.batch * c.in_dim * c.out_dim <= EMULATED_WORK]


# ---------------------------------------------------------------------------------------------------------------------------
# the family
@pytest.mark.parametrize("name", LH.X3_EDGE_NAMES)
def test_planes_generator_meets_its_conditions(name):
    T, U = LH.PLANES_MAX_TERMS, LH.PLANE_UNIT
    for case in LH.x3_edge_table()[name]:
        assert case.mode == MATH_SPLIT_ALL and case.want
        if case.dist != "planes":
            continue
        inp = LH.make_inputs(case)          # (asserts the 48 condition itself)
        gemm_ops = ["x", "w"] + (["g"] if case.kind == "bwd" else [])
        for k in gemm_ops:
            v = inp[k]
            nz = v[v != 0]
            assert nz.size and np.isin(np.abs(nz), [U + 512, U + 513, U - 512, U - 511]).all(), k
            p1, p2, p3 = LH.split3(nz)
            s = np.sign(nz)
            assert (p1 == s * U).all() and (np.abs(p2) == 512).all() and np.isin(p3 * s, [0, 1]).all() and (_f64(p1) + p2 + p3 == nz).all(), k
            assert {-512.0, 512.0} <= set(np.unique(p2 * s)) and {0.0, 1.0} <= set(np.unique(p3 * s)), k
        for k in ("b",) + (("dx0", "dw0") if case.kind == "bwd" else ()):
            assert (inp[k] % U == 0).all() and np.abs(inp[k]).max() <= 2 * U, k
        if case.has(MASK_BY_X):
            assert (inp["x"] >= 0).all() and (inp["x"] == 0).any()
        big = float(max(np.abs(inp[k]).max() for k in gemm_ops))
        assert T * big * big + 3 * U < 2.0 ** 42          # every partial sum, initial contents and bias included
        for gemm, terms in LH.planes_terms(case, inp).items():
            assert terms.max() <= T
            assert terms.max() >= (8 if case.batch <= 1100 else 1), (case.name, gemm, terms.max())          # sums, not single products
        # the non-zero positions use the whole reduction range: every stretch of 32 (a k-tile of the split kernels) holds a pair of non-zero operands
        if case.kind == "fwd":
            used = ((inp["x"] != 0).any(0) & (inp["w"] != 0).any(0))
        elif not case.has(ONLY_DX):
            used = ((inp["g"] != 0).any(1) & (inp["x"] != 0).any(1))
        else:
            used = ((inp["g"] != 0).any(0) & (inp["w"] != 0).any(1))
        k32 = np.add.reduceat(used.astype(int), np.arange(0, used.size, 32))
        assert (k32 > 0).all(), f"{case.name}: {int((k32 == 0).sum())} k-tiles of 32 without a non-zero pair"


def _f64(a):
    return np.asarray(a, np.float64)


def test_the_dropped_products_are_not_zero_on_planes():
    """The expected value differs from the float64 product of the unsplit operands in nearly every output: an exact-fp32 kernel cannot pass."""
    inp = LH.make_inputs(Case("p", "fwd", 1024, 80, 96, NONE, dist="planes", **M3))
    six, true = LH.split_product(inp["x"], inp["w"].T), _f64(inp["x"]) @ _f64(inp["w"]).T
    assert (six != true).mean() > 0.95
    assert (six % LH.PLANE_UNIT == 0).all() and np.abs(six).max() < 2.0 ** 42 and (six.astype(np.float32) == six).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement and its mutants
MUTANTS = {f"a{i}b{j} dropped": dict(pairs=tuple(p for p in SIX if p != (i, j))) for i, j in SIX}
MUTANTS["third plane dropped"] = dict(pairs=tuple(p for p in SIX if 3 not in p))
MUTANTS["a3 paired with b2"] = dict(pairs=tuple((3, 2) if p == (3, 1) else p for p in SIX))
MUTANTS["truncating split"] = dict(rnd=LH.trunc_bf16)

DISC = [Case("disc-fwd", "fwd", 192, 136, 200, RELU, ldy=139, y_off=1, dist="planes", **M3),
        Case("disc-fwd-images", "fwd", 160, 136, 70, NONE, ldx=192, x_off=32, images=("x", "w", "y"), dist="planes", **M3),
        Case("disc-bwd", "bwd", 192, 136, 200, NONE, OVERWRITE, dist="planes", **M3),
        Case("disc-bwd-add-maskx", "bwd", 136, 200, 300, RELU, MASK_BY_X | PREMASKED, images=("w", "dy", "dx"), dist="planes", **M3),
        Case("disc-bwd-live-relu", "bwd", 200, 192, 129, RELU, OVERWRITE, lddx=203, dist="planes", **M3)]


def _run(lib, case):
    be = LH.HostBackend()
    res = (LH.run_fwd if case.kind == "fwd" else LH.run_bwd)(lib, be, case)
    return res, (LH.check_fwd if case.kind == "fwd" else LH.check_bwd)(res)


@pytest.mark.parametrize("name", LH.X3_EDGE_NAMES)
def test_six_product_restatement_passes_the_edge_table(name):
    ran = 0
    for case in _small(LH.x3_edge_table()[name]):
        res, rep = _run(LH.NumpySplitLib(), case)
        assert rep.ok(), f"{case!r}\n{rep}"
        ran += 1
    print(name, ran, "cases;", {k: round(v, 4) for k, v in sorted(LH.WORST.items())})


@pytest.mark.parametrize("case", DISC, ids=[c.name for c in DISC])
def test_checker_accepts_six_products_and_rejects_every_mutant_on_planes(case):
    res, rep = _run(LH.NumpySplitLib(), case)
    assert rep.ok(), str(rep)
    outs = ("y",) if case.kind == "fwd" else ("dw", "dx")
    for what, kw in MUTANTS.items():
        _, rep = _run(LH.NumpySplitLib(**kw), case)
        for out in outs:
            assert any(v.startswith(out + ":") and "exact" in v for v in rep.violations), f"{case.name}: {out} of the mutant '{what}' passes\n{rep}"
        if what == "truncating split" and case.images:      # ... and its images are not the header's
            out = "y" if case.kind == "fwd" else "dx"
            assert any(v.startswith(f"{out} image:") for v in rep.violations), str(rep)


def test_mutants_change_most_outputs_on_planes():
    inp = LH.make_inputs(Case("p", "fwd", 1024, 80, 96, NONE, dist="planes", **M3))
    ref = LH.split_product(inp["x"], inp["w"].T)
    for what, kw in MUTANTS.items():
        frac = float((LH.split_product(inp["x"], inp["w"].T, **kw) != ref).mean())
        print(f"{what}: {100 * frac:.0f} % of the outputs change")
        assert frac > 0.8, what


@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_the_mass_bound_cannot_see_a_dropped_third_plane_on_uniform(kind):
    """Why the family exists: on operands of order one the four products left are within 1e-5 of the mass of the float64 product."""
    case = Case("u", kind, 256, 136, 200, NONE, OVERWRITE if kind == "bwd" else 0, dist="uniform", **M3)
    for what in ("third plane dropped", "a3b1 dropped", "a1b3 dropped"):
        _, rep = _run(LH.NumpySplitLib(**MUTANTS[what]), case)
        assert rep.ok(), f"{what}\n{rep}"
        assert max(rep.worst.values()) < 0.5
    _, rep = _run(LH.NumpySplitLib(**MUTANTS["third plane dropped"]), case.replace(dist="planes"))
    assert not rep.ok()


@pytest.mark.parametrize("seed", range(4))
def test_six_product_restatement_passes_the_random_cases(seed):
    cases = LH.draw_cases_x3(seed)
    assert len(cases) == 6
    for case in cases:
        _, rep = _run(LH.NumpySplitLib(), case)
        assert rep.ok(), f"{case!r}\n{rep}"


def test_generator_reaches_every_distribution_image_and_width_class():
    cases = [c for s in range(8) for c in LH.draw_cases_x3(s)]
    assert {c.dist for c in cases} == {"uniform", "integer", "wide", "planes"} and all(c.mode == MATH_SPLIT_ALL for c in cases)
    assert {n for c in cases for n in c.images} == set(LH.IMAGE_NAMES) and any(not c.images for c in cases)
    assert sum(c.planes_exact for c in cases) >= 8 and sum(not c.x3_layer for c in cases) >= 6
    assert {c.kind for c in cases if c.planes_exact} == {"fwd", "bwd"}


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle library in this mode: unsplit fp32 products.  The harness (images, sentinels, the mode's clean-up) on a real library
ORACLE_CASES = [c for n in ("x3-v2w8-fwd", "x3-v2w8-dx", "x3-dw-128", "x3-narrow-layers") for c in _small(LH.x3_edge_table()[n]) if not c.planes_exact]
ORACLE_CASES += [Case("o-fwd-images", "fwd", 160, 136, 70, RELU, ldx=192, x_off=32, ldy=139, y_off=1, images=("x", "w", "y"), **M3),
                 Case("o-bwd-images", "bwd", 136, 200, 77, SIG, 0, lddy=203, dy_off=2, images=("x", "w", "y", "dy", "dx"), stale=("dy",), **M3)]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.name for c in ORACLE_CASES])
def test_oracle_passes_the_other_distributions(olib, case):
    res, rep = LH.run_and_check_x3(olib, LH.HostBackend(), case, LH.TABLE_CUS)
    assert rep.ok(), f"{case!r}\n{rep}"
    assert all(im.untouched() for n, im in res.twins.items() if n not in res.twin_inputs)      # the oracle's GEMMs keep no image


def test_oracle_is_rejected_on_planes(olib):
    for case in DISC[:1] + DISC[2:3]:
        _, rep = _run(olib, case)
        assert any("exact" in v for v in rep.violations), f"{case.name}: an exact-fp32 product passes for the six-product sum"
        _, rep = _run(olib, case.replace(in_dim=127, ldx=None, lddx=None))      # a narrow layer is the fp32 kernels': the bound against the unsplit product
        assert rep.ok(), str(rep)


def test_the_mode_and_the_regions_do_not_outlive_a_call(olib, monkeypatch):
    lib = LH.NumpySplitLib()

    def boom(*a):
        raise RuntimeError("after the call, before the clean-up")
    with monkeypatch.context() as m:
        m.setattr(LH, "_finish", boom)
        with pytest.raises(RuntimeError):
            LH.run_fwd(lib, LH.HostBackend(), DISC[1])
    assert lib.mode == 0 and not lib.regions


# ---------------------------------------------------------------------------------------------------------------------------
# ImageBuf on its own
def _image(ld=45, off=35, rows=7, cols=40):
    be = LH.HostBackend()
    data = (np.random.default_rng(5).uniform(-1, 1, (rows, cols)) * 2.0 ** np.random.default_rng(6).integers(-12, 12, (rows, cols))).astype(np.float32)
    buf = LH.Buf(be, rows, cols, ld, off, data)
    return buf, LH.ImageBuf(be, buf), data


def test_imagebuf_layout_alignment_and_fill(olib):
    buf, im, data = _image()
    n = buf.valid.size
    assert buf.be.addr(buf.h) % 128 == 0 and im.base % 128 == 0 and im.before.size * 2 == (4 * n + 127) // 128 * 192
    assert (im.before == LH.SENTINEL16).all() and im.valid.sum() == 3 * data.size
    base = im.register(olib)
    try:
        im.fill(olib).fetch()
    finally:
        olib.lib.ffh_ctx_bf16x3_mirror_set(olib.ctx, base, 4 * n, None)
    assert (im.host[~im.valid] == LH.SENTINEL16).all() and not im.problems("x", data, must_write=True)
    # element e has its term p at byte (e / 32) * 192 + p * 64 + (e % 32) * 2 (include/ff_hip.h), written out by hand for one element
    r, c = 4, 17
    e = buf.off + r * buf.ld + c
    x1 = LH.rne_bf16(data[r, c:c + 1])
    x2 = LH.rne_bf16(data[r, c:c + 1] - x1)
    x3 = LH.rne_bf16(data[r, c:c + 1] - x1 - x2)
    for p, term in enumerate((x1, x2, x3)):
        at = ((e // 32) * 192 + p * 64 + (e % 32) * 2) // 2
        assert im.host[at] == term.view(np.uint32)[0] >> 16
    im.snapshot()
    assert im.fetch().untouched() and not im.problems("x")
    im.poison().fetch()
    assert (im.host[im.valid] == 0x7FC0).all() and (im.host[~im.valid] == LH.SENTINEL16).all()


def test_imagebuf_reports_swapped_planes_padding_a_stale_element_and_an_unwritten_image():
    buf, im, data = _image()
    im.fetch()
    assert not im.problems("y", data) and im.problems("y", data, must_write=True), "an unwritten image on a bf16x3 route went unnoticed"
    good = im.before.copy()
    good[im.at] = LH.plane_bits(data)
    im.host = good.copy()
    assert not im.problems("y", data, must_write=True)
    im.host = good.copy()
    im.host[im.at[1]], im.host[im.at[2]] = good[im.at[2]], good[im.at[1]]          # the second and the third plane swapped
    assert any("term 2" in p for p in im.problems("y", data))
    places = {"offset": LH.image_at(0), "padding column": LH.image_at(buf.flat_index(2, 40)) + 32, "tail": LH.image_at(buf.valid.size - 1) + 64,
              "the rest of the last group": good.size - 1}
    for what, at in places.items():
        assert not im.valid[at], what
        im.host = good.copy()
        im.host[at] = 0x3F80
        assert any("outside the valid block" in p for p in im.problems("y", data)), what
    im.host = good.copy()
    im.host[im.at[2, 41]] = LH.SENTINEL16                                            # one element's third term left as it was: stale
    assert any("term 3 of (1, 1)" in p for p in im.problems("y", data))
    im.host = good.copy()
    im.host[im.at[0, 5 * 40:6 * 40]] = good[im.at[0, 4 * 40:5 * 40]]                  # row 5 holds row 4's first terms
    assert any("(5, 0)" in p for p in im.problems("y", data))
    im.host = good.copy()
    im.host[im.at] = LH.plane_bits(data, LH.trunc_bf16)                               # a truncating split
    assert im.problems("y", data)
    im.host = good.copy()
    assert any("input" in p for p in im.problems("x"))                               # an input's image has to stay as it was


def test_checker_reports_an_image_written_by_the_wrong_rule_on_a_result():
    """Through check_fwd / check_bwd, the result marked as the HIP library's: an untouched output image under a bf16x3 / x3_dma route."""
    case = DISC[1]
    res, rep = _run(LH.NumpySplitLib(write_images=False), case)
    assert rep.ok()
    res.is_hip = True
    for route in ("linear_fwd gemm (bf16)|bf16x3_128x128|splitk=1|v2w8", "linear_fwd gemm (bf16)|x3_dma_256x256_planes|splitk=1"):
        res.route = route
        assert any(v.startswith("y image: not written") for v in LH.check_fwd(res).violations)
    res.route = "linear_fwd gemm|f32_32x32_cfg2|splitk=1"
    assert LH.check_fwd(res).ok()
    res, rep = _run(LH.NumpySplitLib(), case)
    res.is_hip, res.route = True, "linear_fwd gemm (bf16)|bf16x3_128x128|splitk=1|v2w8"
    assert LH.check_fwd(res).ok() and not res.twins["y"].untouched()
    res.twins["x"].host = res.twins["x"].host.copy()
    res.twins["x"].host[res.twins["x"].at[2, 3]] ^= 0x10
    assert any(v.startswith("x image:") for v in LH.check_fwd(res).violations)
    bwd = DISC[3]
    res, rep = _run(LH.NumpySplitLib(write_images=False), bwd)
    res.is_hip, res.route = True, "linear_bwd dw gemm (bf16)|bf16x3_128x128|splitk=2|mfma32;linear_bwd dx gemm (bf16)|bf16x3_128x128|splitk=1|v2w8"
    assert any(v.startswith("dx image: not written") for v in LH.check_bwd(res).violations)
    res.route = "linear_bwd dw gemm (bf16)|bf16x3_128x128|splitk=2|mfma32"
    assert LH.check_bwd(res).ok()


def test_a_run_without_images_is_compared_bit_for_bit(monkeypatch):
    """run_and_check_x3: y of the run with images against y of the run without."""
    class Drifting(LH.NumpySplitLib):
        def ffh_linear_fwd(self, *a):
            rc = super().ffh_linear_fwd(*a)
            if self.regions:
                y00 = self._view(a[3], 1, 1, 1)
                y00[0, 0] = np.nextafter(y00[0, 0], np.float32(np.inf))          # one ulp: inside the bound, the image consistent with it
                self._image(a[3], a[9], a[8], a[4])
            return rc
    be = LH.HostBackend()
    monkeypatch.setattr(be, "is_hip", True, raising=False)
    monkeypatch.setattr(LH.NumpySplitLib, "ffh_linear_last_route", lambda self, ctx: b"linear_fwd gemm (bf16)|bf16x3_128x128|splitk=1|v2w8")
    case = DISC[1].replace(dist="uniform")
    _, rep = LH.run_and_check_x3(LH.NumpySplitLib(), be, case, LH.TABLE_CUS, routes=False)
    assert rep.ok(), str(rep)
    _, rep = LH.run_and_check_x3(Drifting(), be, case.replace(act=NONE, bias=False), LH.TABLE_CUS, routes=False)
    assert any("differs between the run with images" in v for v in rep.violations), str(rep)


# ---------------------------------------------------------------------------------------------------------------------------
# the route model
def test_route_model_reaches_every_want_and_the_table_names_every_kernel():
    toks = set()
    for name, cases in LH.x3_edge_table(LH.TABLE_CUS).items():
        dists = {c.dist for c in cases}
        assert "planes" in dists and dists & {"uniform", "wide"}, f"{name}: {dists}"
        for case in cases:
            assert case.want, f"{case.name} names no kernel"
            assert not LH.model_reaches(case), f"{case.name}: the route model gives {LH.expected_route(case, LH.TABLE_CUS)}, the case is there for {case.want}"
            toks.update((t, case.planes_exact) for t in LH.expected_route(case, LH.TABLE_CUS)[0])
    for kernel, sub in LH.X3_KERNELS.items():
        assert any(sub in t for t, _ in toks), f"no case on {kernel}"
        assert any(sub in t and exact for t, exact in toks), f"no 'planes' case on {kernel}"
    names = {t for t, _ in toks}
    F, DW, DX, DXM = "linear_fwd gemm (bf16)|", "linear_bwd dw gemm (bf16)|", "linear_bwd dx gemm (bf16)|", "linear_bwd dx gemm (bf16, masking)|"
    S = "bf16x3_128x128|splitk="
    assert {F + S + "1|v2w8", F + S + "1|v2w4", DX + S + "1|v2w8", DX + S + "1|v2w4", DXM + S + "1|v2w8", DXM + S + "1|v2w4", DW + S + "1|mfma32", DW + S + "2|mfma32",
            DW + S + "3|mfma32", DW + S + "5|mfma32", DW + "bf16x3_256x256|splitk=8", F + "x3_dma_256x256_planes", F + "x3_dma_256x256_planes+image",
            DX + "x3_dma_256x256_planes", DX + "x3_dma_256x256_planes+image", DW + "x3_dma_256x256_planes", DW + "x3_dma_256x256_planes|slots"} <= names, sorted(names)


def test_route_tokens_of_the_library_normalize_to_the_models():
    r = ("linear_bwd dw gemm (bf16)|x3_dma_256x256_planes|splitk=64|slots;linear_bwd dx gemm (bf16)|x3_dma_256x256_planes+image|splitk=1;"
         "linear_bwd dw gemm (bf16)|bf16x3_128x128|splitk=3|mfma32;linear_fwd gemm (bf16)|bf16x3_128x128|splitk=1|v2w8;linear_bwd dw gemm (bf16)|bf16x3_256x256|splitk=8")
    assert LH.normalize_route(r) == ["linear_bwd dw gemm (bf16)|x3_dma_256x256_planes|slots", "linear_bwd dx gemm (bf16)|x3_dma_256x256_planes+image",
                                     "linear_bwd dw gemm (bf16)|bf16x3_128x128|splitk=3|mfma32", "linear_fwd gemm (bf16)|bf16x3_128x128|splitk=1|v2w8",
                                     "linear_bwd dw gemm (bf16)|bf16x3_256x256|splitk=8"]
    assert LH.x3_dma_splits(r) == [("linear_bwd dw gemm (bf16)|x3_dma_256x256_planes|splitk=64|slots", 64), ("linear_bwd dx gemm (bf16)|x3_dma_256x256_planes+image|splitk=1", 1)]


def test_dma_serve_conditions_one_by_one():
    """Each condition of launch_gemm_x3_dma the table's "declined" group names, flipped alone on the forward the kernel serves."""
    base = Case("s", "fwd", 128, 1000, 12200, RELU, ldy=1024, images=("x", "w", "y"), **M3)
    tok = lambda c, cus=256: LH.expected_route(c, cus)[0][0]
    assert tok(base).endswith("x3_dma_256x256_planes+image")
    for kw in (dict(x_off=8, ldx=160), dict(w_off=4), dict(ldx=132), dict(in_dim=136, ldx=160), dict(out_dim=1004), dict(images=("x", "y")), dict(images=("w", "y")),
               dict(ldy=1022), dict(y_off=2), dict(bias_off=1), dict(batch=12032)):
        assert "bf16x3_128x128|splitk=1|v2w4" in tok(base.replace(**kw)), kw
    for kw in (dict(y_off=4), dict(ldy=1000), dict(images=("x", "w")), dict(y_off=32 + 4)):
        assert tok(base.replace(**kw)).endswith("x3_dma_256x256_planes"), kw
    assert tok(base.replace(y_off=32)).endswith("+image")
    assert "v2w4" in tok(base, 260) and tok(base, 255).endswith("+image")          # 192 tiles: 75 % of 256 CUs
    dx = Case("s", "bwd", 992, 128, 12200, NONE, ONLY_DX | MASK_BY_X, images=("w", "dy", "dx"), **M3)
    assert tok(dx).endswith("+image") and "v2w4" in tok(dx.replace(x_off=2, ldx=996)) and "v2w4" in tok(dx.replace(ldx=994)) and "v2w4" in tok(dx.replace(act=SIG))
    dw = Case("s", "bwd", 192, 264, 16384, NONE, ONLY_DW, lddy=288, images=("x", "dy"), **M3)
    assert tok(dw).endswith("planes|slots") and tok(dw.replace(scratch=False)).endswith("planes")
    assert "mfma32" in tok(dw.replace(batch=16352)) and "mfma32" in tok(dw.replace(det=True)) and "mfma32" in tok(dw.replace(out_dim=256, lddy=256, in_dim=256, ldx=256))
    assert "mfma32" in tok(dw.replace(dy_off=2)) and tok(dw.replace(dy_off=32)).endswith("|slots") and "mfma32" in tok(dw.replace(out_dim=262))
    assert tok(dw.replace(out_dim=262, db=False)).endswith("|slots")                 # out_dim % 4 matters to the bias gradient only
    assert LH.x3_dma_dw_split(256, 2, 512) == 64 and LH.x3_dma_dw_split(256, 2, 511) is None and LH.x3_dma_dw_split(256, 6, 176) == 22
