"""bf16 embedding tables at the model level (--embedding-dtype / --embedding-rounding), host logic on the CPU: the flags, the
compile() refusals (in child processes, with the CPU oracle as kernel library -- no GPU is opened) and the C API / ctypes surface.
The GPU side (the numbers a bf16-table model computes) is tests/test_gpu_bf16_model.py."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from dlrm_flexflow_amd import build, ffmodel

EXE = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "dlrm_testing")
HOST_LIB = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "libffmodel.so")
HEADER = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "ffmodel_c.h")
SMALL = ["-b", "64", "--arch-sparse-feature-size", "8", "--arch-embedding-size", "100-200-50", "--arch-mlp-bot", "13-16-8",
         "--arch-mlp-top", "32-16-1", "--data-size", "128", "--epochs", "1"]
NEW_C_API = ["flexflow_config_set_embedding_dtype", "flexflow_config_set_embedding_rounding", "flexflow_tensor_set_bf16",
             "flexflow_tensor_get_bf16", "flexflow_tensor_get_data_type"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


def _oracle():
    import dlrm_helpers as H
    return H.oracle_backend()


def _driver(*extra):
    return subprocess.run([EXE, "--backend", _oracle(), *SMALL, *extra], capture_output=True, text=True, timeout=300)


def test_driver_refuses_bf16_tables_on_a_library_without_the_extension():
    """The oracle exports include/ff_hip.h but not include/ff_hip_bf16.h: the driver dies in compile() with the reason instead of
    ignoring the flag and training fp32 tables."""
    r = _driver("--embedding-dtype", "bf16")
    assert r.returncode != 0
    assert "without the bf16 extension" in r.stderr and "--embedding-dtype fp32" in r.stderr, r.stderr[-2000:]
    r = _driver("--embedding-dtype=bf16", "--embedding-rounding=nearest")     # the one-token form
    assert r.returncode != 0 and "without the bf16 extension" in r.stderr, r.stderr[-2000:]


def test_driver_with_fp32_tables_spelled_out_still_trains():
    r = _driver("--embedding-dtype", "fp32", "--embedding-rounding", "nearest")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "THROUGHPUT" in r.stdout


@pytest.mark.parametrize("flag,value", [("--embedding-dtype", "fp16"), ("--embedding-dtype", "float"), ("--embedding-rounding", "up"),
                                        ("--embedding-rounding", "")])
def test_bad_flag_values_are_refused(flag, value):
    r = _driver(f"{flag}={value}")
    assert r.returncode != 0
    assert f"{flag} {value}:" in r.stderr, r.stderr[-2000:]


_REFUSAL = r"""
import sys
sys.path.insert(0, {tests!r})
import dlrm_helpers as H
case = {case!r}
bf16 = ["--embedding-dtype", "bf16"]
if case == "row_sharded":
    import os, torch.distributed as dist
    from dlrm_flexflow_amd.comm import TorchComm
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % (33400 + os.getpid() % 1000), rank=0, world_size=1)
    comm = TorchComm(on_gpu=False)
    H.build_golden_dlrm(H.oracle_backend(), comm=comm.struct, force_exchange=True, row_shard_rows=1, extra_argv=bf16)
elif case == "dense_update":
    H.build_golden_dlrm(H.oracle_backend(), dense_update=True, extra_argv=bf16)
elif case == "momentum":
    H.build_golden_dlrm(H.oracle_backend(), sgd=H.MOM_HP, extra_argv=bf16)
elif case == "momentum_sparse":
    H.build_golden_dlrm(H.oracle_backend(), sgd=H.MOM_HP, extra_argv=bf16 + ["--sparse-embedding-optimizer"])
elif case == "adam_sparse":
    H.build_golden_dlrm(H.oracle_backend(), adam=H.ADAM_HP, extra_argv=bf16 + ["--sparse-embedding-optimizer"])
print("COMPILED")
"""


@pytest.mark.parametrize("case,message", [
    ("row_sharded", "is row-sharded; bf16 tables are table-wise for now: drop --row-shard-rows"),
    ("dense_update", "needs the fused sparse table update: drop --dense-embedding-update"),
    ("momentum", "with momentum / weight-decay SGD or Adam needs --sparse-embedding-optimizer"),
])
def test_compile_refuses_what_the_bf16_update_does_not_cover(case, message):
    """Each case dies in compile() with its reason and the flag to change, before the library check and before anything is
    allocated or launched (the oracle would otherwise refuse first for want of the extension)."""
    src = _REFUSAL.format(tests=os.path.join(ROOT, "tests"), case=case)
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "COMPILED" not in r.stdout
    assert message in r.stderr, r.stderr[-2000:]
    assert "without the bf16 extension" not in r.stderr


@pytest.mark.parametrize("case", ["momentum_sparse", "adam_sparse"])
def test_sparse_momentum_and_adam_are_accepted_on_bf16_tables(case):
    """With --sparse-embedding-optimizer momentum and Adam pass every optimizer check: on the oracle compile() stops only at the library."""
    src = _REFUSAL.format(tests=os.path.join(ROOT, "tests"), case=case)
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "without the bf16 extension" in r.stderr, r.stderr[-2000:]


def test_python_config_rejects_bad_values():
    cfg = ffmodel.FFConfig(argv=["-b", "16"])
    cfg.set(embedding_dtype="bf16", embedding_rounding="nearest")
    cfg.set(embedding_dtype="fp32", embedding_rounding="stochastic")
    with pytest.raises(ValueError):
        cfg.set(embedding_dtype="fp16")
    with pytest.raises(ValueError):
        cfg.set(embedding_rounding="down")


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_new_c_api_is_declared_exported_and_bound():
    """The new functions are in ffmodel_c.h, exported by libffmodel.so, and bound in ffmodel.py with as many arguments as the
    header gives them."""
    hdr = open(HEADER).read()
    exp = _exported(HOST_LIB)
    L = ffmodel.lib()
    for name in NEW_C_API:
        m = re.search(r"\b" + name + r"\(([^)]*)\)", hdr)
        assert m, f"{name} is not declared in ffmodel_c.h"
        assert name in exp, f"{name} is not exported"
        nargs = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert len(getattr(L, name).argtypes) == nargs, name
    assert ffmodel.DT_BF16 == int(re.search(r"DT_BF16 = (\d+)", open(os.path.join(ROOT, "dlrm_flexflow_amd", "host", "ffmodel.h")).read()).group(1))
