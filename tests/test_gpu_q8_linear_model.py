"""GPU test (-m gpu) of --eval-mlp-dtype int8 through the host model: 64 -> 128 relu -> 64 relu -> 1 sigmoid.  The first two layers
have an int8 image, the last keeps fp32.  What eval_batch() leaves in a layer's output is the numpy restatement of the rule on that layer's input and
parameters, bit for bit; the images are re-quantized once after a step, not per batch; training is the fp32 run's to the bit."""
import numpy as np

import pytest

from dlrm_flexflow_amd import capi, ffmodel

pytestmark = pytest.mark.gpu
B = 96


def _run(dtype):
    cfg = ffmodel.FFConfig(argv=["-b", str(B), "--eval-batches", "1", "--deterministic"], backend=capi.HIP_LIB_PATH).set(eval_mlp_dtype=dtype)
    m = ffmodel.FFModel(cfg)
    x = m.create_tensor([B, 64], ffmodel.DT_FLOAT)
    m.dense(m.dense(m.dense(x, 128, capi.AC_MODE_RELU), 64, capi.AC_MODE_RELU), 1, capi.AC_MODE_SIGMOID)
    m.set_sgd_optimizer(lr=0.5)
    m.compile(ffmodel.LOSS_BCE, (ffmodel.METRICS_ACCURACY, ffmodel.METRICS_AUC))
    m.init_layers()
    rng = np.random.default_rng(3)
    xs = rng.standard_normal((B, 64)).astype(np.float32)
    x.set(xs)
    m.label_tensor.set((rng.random((B, 1)) > 0.5).astype(np.float32))
    int8 = dtype == "int8"
    count = lambda: (m.counter("q8_linear_quantize_launches"), m.counter("q8_linear_gemm_launches"))

    def check_layers():
        """both int8 layers against the rule, from the values the model itself holds"""
        m.sync()
        inputs = [xs, m.layer_output(0).get()]
        for li in (0, 1):
            want = ffmodel.q8_linear_reference(inputs[li], m.parameter(li, 0).get(), m.parameter(li, 1).get(), capi.AC_MODE_RELU)
            assert np.array_equal(m.layer_output(li).get().view(np.uint32), want.view(np.uint32)) == int8, (dtype, li)

    m.eval_batch()
    check_layers()
    assert count() == ((1, 2) if int8 else (0, 0))
    m.eval_batch()                                                   # nothing wrote a kernel: the images are current
    assert count() == ((1, 4) if int8 else (0, 0))
    w_before = m.parameter(1, 0).get()
    m.forward(); m.zero_gradients(); m.backward(); m.update()
    m.eval_batch()
    assert count() == ((2, 6) if int8 else (0, 0))
    assert not np.array_equal(m.parameter(1, 0).get(), w_before)
    check_layers()                                                   # ... with the new weights
    m.sync()
    params = [m.parameter(li, k).get() for li in range(3) for k in (0, 1)]
    m.close()
    return params


def test_eval_batch_runs_the_rule_and_training_is_untouched(hip):
    got, ref = _run("int8"), _run("fp32")
    for a, b in zip(got, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
