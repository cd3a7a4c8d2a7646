"""GPU tests (-m gpu) of bf16 embedding tables at the model level (--embedding-dtype bf16): a bf16-table model against the fp32-table
model built from the same seed, bit for bit.  Before each step the fp32 model's tables are loaded with the widened bf16 tables, so both
steps see the same numbers: the predictions and MLP weights must be identical and every bf16 table must be the rounding
(include/ffh_bf16.h, tests/bf16_helpers.py) of the fp32 model's updated table.  --deterministic: without it the weight gradients use
floating-point atomics and two runs are not bit-identical.  The refusals are tested on the CPU (tests/test_bf16_model_cpu.py)."""
import numpy as np
import pytest

from dlrm_flexflow_amd import capi, ffmodel
import bf16_helpers as BH
import dlrm_helpers as H

pytestmark = pytest.mark.gpu

HIP = capi.HIP_LIB_PATH
BF16 = ["--embedding-dtype", "bf16"]


def _seed(config_seed=0):
    """The rounding seed of a model: ffh_hash(FFConfig::seed, 0xBF16) (FFModel::bf16_rounding)."""
    return int(BH.hash64(np.uint64(config_seed), np.uint64(0xBF16)))


def _tables(m, h):
    return [(k, m.parameter(li, 0)) for k, li in h["names"].items() if k.startswith("emb")]


def _step(m, h, trace):
    if trace:
        m.begin_trace(7)
    m.forward(); m.zero_gradients(); m.backward(); m.update()
    if trace:
        m.end_trace(7)
    m.sync()
    return m.layer_output(h["final"]).get()


def _compare(mode, trace=False, overlap=True, flags=(), steps=3, early_sort=None, **opt):
    common = ["--deterministic"] + list(flags)
    m32, h32 = H.build_golden_dlrm(HIP, enable_graph=trace, overlap=overlap, extra_argv=common, **opt)
    m16, h16 = H.build_golden_dlrm(HIP, enable_graph=trace, overlap=overlap, **opt,
                                   extra_argv=common + BF16 + ["--embedding-rounding", "nearest" if mode == BH.ROUND_NEAREST else "stochastic"])
    t32, t16 = _tables(m32, h32), _tables(m16, h16)
    for (k, p) in t16:
        assert p.data_type == ffmodel.DT_BF16, k
    for k, p in t32:
        assert p.data_type == ffmodel.DT_FLOAT, k
    g = h32["g"]
    for (k, p) in t16:                                        # set_weights on a bf16 table: nearest even of the fp32 values
        assert np.array_equal(p.get(raw_bf16=True), BH.rne(g[f"init/{k}.weight"])), k
    for step in range(steps):
        for (k, p32), (_, p16) in zip(t32, t16):
            p32.set(BH.widen(p16.get(raw_bf16=True)))
        y32, y16 = _step(m32, h32, trace), _step(m16, h16, trace)
        assert np.array_equal(y32.view(np.uint32), y16.view(np.uint32)), f"predictions, step {step}"
        for k, li in h32["names"].items():
            if k.startswith("emb"):
                continue
            for j in (0, 1):
                a, b = m32.parameter(li, j).get(), m16.parameter(h16["names"][k], j).get()
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{k}[{j}] step {step}"
        for t, ((k, p32), (_, p16)) in enumerate(zip(t32, t16)):
            want = BH.round_table(p32.get(), mode, _seed(), it=step, table=t, col0=0)
            got = p16.get(raw_bf16=True)
            assert np.array_equal(got, want), f"{k} step {step}: {np.count_nonzero(got != want)} of {got.size} differ"
            assert np.array_equal(p16.get(), BH.widen(got))     # get_float widens exactly
    assert m16.counter("bf16_updates") == steps
    if early_sort is not None:                                # the early sort ran (sort-only launches behind the gather), or did not
        assert (m16.counter("early_sorts") > 0) == early_sort and (m32.counter("early_sorts") > 0) == early_sort
    m32.close(); m16.close()


@pytest.mark.parametrize("trace,overlap,flags,early", [
    (False, True, ["--early-sort"], True),
    (False, True, ["--no-early-sort"], False),
    (False, False, [], False),
    (True, True, [], None),
    (False, True, ["--fp32-split-bf16x3"], None),
])
def test_bf16_model_equals_rne_of_the_fp32_model(hip, trace, overlap, flags, early):
    _compare(BH.ROUND_NEAREST, trace=trace, overlap=overlap, flags=flags, early_sort=early)


@pytest.mark.parametrize("opt", [dict(sgd=dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-3)), dict(adam=H.ADAM_HP)],
                         ids=["momentum", "adam"])
@pytest.mark.parametrize("mode", [BH.ROUND_NEAREST, BH.ROUND_STOCHASTIC], ids=["nearest", "stochastic"])
def test_sparse_momentum_and_adam_on_bf16_tables(hip, opt, mode):
    """--sparse-embedding-optimizer on bf16 tables (ffh_embedding_bwd_opt_*_multi_bf16): the fp32 state of both models evolves on the same
    widened tables, so any difference in it shows in the next step's table bits; checked over three steps (early sort on: sort + apply)."""
    _compare(mode, flags=["--sparse-embedding-optimizer", "--early-sort"], early_sort=True, **opt)


@pytest.mark.parametrize("trace", [False, True])
def test_bf16_model_stochastic_equals_round_table_of_the_fp32_model(hip, trace):
    """The stochastic bits are keyed by the counter, advanced once per step: a replayed graph draws fresh bits each step."""
    _compare(BH.ROUND_STOCHASTIC, trace=trace)


def test_stochastic_eager_equals_traced(hip):
    out = []
    for trace in (False, True):
        m, h = H.build_golden_dlrm(HIP, enable_graph=trace, extra_argv=["--deterministic"] + BF16)
        for _ in range(3):
            _step(m, h, trace)
        out.append([p.get(raw_bf16=True) for _, p in _tables(m, h)])
        assert m.counter("bf16_updates") == 3
        m.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def _tiny_model(dtype, init, rows=1000, D=16, B=32, seed=11):
    cfg = ffmodel.FFConfig(argv=["-b", str(B), "--seed", str(seed)], backend=HIP)
    cfg.set(embedding_dtype=dtype)
    m = ffmodel.FFModel(cfg)
    s = m.create_tensor([B, 1], ffmodel.DT_INT64)
    x = m.create_tensor([B, D], ffmodel.DT_FLOAT)
    e = m.embedding(s, rows, D, capi.AGGR_MODE_SUM, kernel_initializer=init(m))
    z = m.concat([x, e], 1)
    m.dense(z, 1, capi.AC_MODE_SIGMOID)
    m.set_sgd_optimizer(lr=0.01)
    m.compile()
    m.init_layers()
    return m, m.parameter(0, 0)


@pytest.mark.parametrize("init", [lambda m: m.uniform_initializer(5, -0.05, 0.05), lambda m: m.norm_initializer(6, 0.0, 0.3),
                                  lambda m: m.zero_initializer(), lambda m: m.glorot_uniform_initializer(7)],
                         ids=["uniform", "norm", "zero", "glorot"])
def test_init_is_the_nearest_even_rounding_of_the_fp32_init(hip, init):
    m32, p32 = _tiny_model("fp32", init)
    m16, p16 = _tiny_model("bf16", init)
    assert p16.data_type == ffmodel.DT_BF16
    assert np.array_equal(p16.get(raw_bf16=True), BH.rne(p32.get()))
    m32.close(); m16.close()


def test_weights_api_rounds_widens_and_copies_raw_bits(hip):
    m, p = _tiny_model("bf16", lambda m: m.zero_initializer())
    R, D = p.dims
    rng = np.random.default_rng(3)
    w = rng.standard_normal((R, D)).astype(np.float32)
    w.reshape(-1)[:len(BH.edge_values())] = BH.edge_values()
    p.set(w)                                                    # fp32 in: nearest even
    assert np.array_equal(p.get(raw_bf16=True), BH.rne(w))
    assert np.array_equal(p.get().view(np.uint32), BH.widen(BH.rne(w)).view(np.uint32))   # fp32 out: exact widening
    bits = rng.integers(0, 1 << 16, (R, D), dtype=np.uint16)
    p.set(bits, raw_bf16=True)                                  # raw bits round-trip
    assert np.array_equal(p.get(raw_bf16=True), bits)
    m.close()
