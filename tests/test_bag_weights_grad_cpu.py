"""The gradient of per-sample bag weights (include/ffh_bag_weights_grad.h) without a GPU: the surface of the extension, and compile() on the CPU
oracle -- which has neither weighted form -- for a model whose weights an operator produces: every run ends in a refusal."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from dlrm_flexflow_amd import capi
import dlrm_helpers as H

EXT = capi.EXTENSIONS["bag_weights_grad"]
# a table whose weights are sigmoid(Linear(dense -> 3)), built through the Python API in a process of its own (compile() ends the process)
MODEL = """import sys
from dlrm_flexflow_amd import capi, ffmodel
m = ffmodel.FFModel(ffmodel.FFConfig(argv=["-b", "8"] + sys.argv[3:], backend=sys.argv[1]))
ids, dense = m.create_tensor([8, 3], ffmodel.DT_INT64), m.create_tensor([8, 4], ffmodel.DT_FLOAT)
gate = m.dense(dense, 3, capi.AC_MODE_SIGMOID)
z = m.concat([m.dense(dense, 4, capi.AC_MODE_RELU), m.embedding(ids, 20, 4, int(sys.argv[2]), per_sample_weights=gate)], 1)
m.dense(z, 1, capi.AC_MODE_SIGMOID)
m.set_sgd_optimizer(lr=0.1)
m.compile()
print("COMPILED")
"""


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_library_exports_the_extension_and_the_oracle_does_not(oracle):
    from dlrm_flexflow_amd import build
    syms = EXT.header_symbols()
    assert set(syms) == set(capi._SIGS_BAG_WEIGHTS_GRAD) and len(syms) == len(set(syms)) == 4
    body = open(EXT.header_path).read().split("#define FFH_BAG_WEIGHTS_GRAD_API_LIST")[0]
    assert set(re.findall(r"\b(ffh_[a-z0-9_]+)\s*\(", body)) == set(syms)      # every declared function is in the list
    assert not [s for s in syms if s not in _exported(build.build_hip())]
    assert ctypes.CDLL(capi.HIP_LIB_PATH, mode=ctypes.RTLD_LOCAL).ffh_bag_weights_grad_abi_version() == EXT.header_abi_version() == 1      # loads without a GPU
    assert not set(syms) & _exported(oracle.ORACLE_LIB) and not hasattr(capi, "BAG_WEIGHTS_GRAD_HEADER_PATH")
    with_list = [p for p in glob.glob(os.path.join(ROOT, "include", "ff_hip_*.h")) if re.search(r"#define FFH_\w+_API_LIST\(X\)", open(p).read())]
    assert len(with_list) == 15                                                # the registry still holds the fifteen ff_hip_* headers
    o = capi.FFHLib(oracle.ORACLE_LIB)
    with pytest.raises(capi.FFHError, match="no bag-weights-grad extension.*include/ffh_bag_weights_grad.h"):
        capi.bag_weights_grad_api(o)
    o.close()


@pytest.mark.parametrize("aggr,argv,names", [
    (capi.AGGR_MODE_SUM, [], ["include/ffh_bag_weights_grad.h", "bag-weights-grad extension", "--backend"]),
    (capi.AGGR_MODE_AVG, [], ["AGGR_MODE_AVG", "drop --embedding-pooling mean"]),
    (capi.AGGR_MODE_SUM, ["--dense-embedding-update"], ["drop --dense-embedding-update"]),
    (capi.AGGR_MODE_SUM, ["--no-ragged-gather"], ["drop --no-ragged-gather"]),
    (capi.AGGR_MODE_SUM, ["--no-ragged-update"], ["drop --no-ragged-update"]),
    (capi.AGGR_MODE_SUM, ["--eval-embedding-dtype", "int8"], ["drop --eval-embedding-dtype int8"]),
    (capi.AGGR_MODE_SUM, ["--async-launch"], ["drop --async-launch"]),
])
def test_compile_refuses_operator_produced_weights(aggr, argv, names):
    r = subprocess.run([sys.executable, "-c", MODEL, H.oracle_backend(), str(aggr), *argv], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode != 0 and "COMPILED" not in r.stdout, r.stdout[-1000:]
    for n in names + ["per-sample weights"]:
        assert n in r.stderr, (n, r.stderr[-2000:])
    assert "--embedding-per-sample-weights" not in r.stderr      # no driver flag built this model: the advice is to pass no per_sample_weights
