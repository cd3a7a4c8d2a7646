"""CPU tests of the wide dot interaction's host side (include/ffh_dot_wide.h): a kernel library without the extension -- the CPU oracle -- serves
--arch-interaction-op dot-tril up to 32 feature vectors as before and refuses more with a message that says what to use instead."""
import signal
import subprocess
import sys

import pytest

from conftest import ROOT
import dlrm_helpers as H


def _build(tables):
    """A Python child that builds and compiles a dot-tril model of `tables` tables on the oracle and does nothing else."""
    c = tables + 1
    args = ["--backend", H.oracle_backend(), "-b", "8", "--arch-sparse-feature-size", "4", "--arch-embedding-size", "-".join(["10"] * tables),
            "--arch-mlp-bot", "3-4", "--arch-mlp-top", f"{4 + c * (c - 1) // 2}-4-1", "--arch-interaction-op", "dot-tril", "--data-size", "8"]
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from dlrm_flexflow_amd import ffmodel\n"
            "app = ffmodel.DLRM(%r)\n"
            "print('BUILT', app.model.num_layers)\n" % (ROOT, args))
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("tables,builds", [(31, True), (33, False)])
def test_the_oracle_serves_dot_tril_up_to_32_feature_vectors(tables, builds):
    r = _build(tables)
    if builds:
        assert r.returncode == 0 and "BUILT" in r.stdout and "FATAL" not in r.stderr, r.stderr[-2000:]
        assert "wide kernel" not in r.stdout
    else:
        assert r.returncode == -signal.SIGABRT, (r.returncode, r.stderr[-2000:])
        fatal = [l for l in r.stderr.splitlines() if l.startswith("FATAL")]
        assert len(fatal) == 1 and "include/ffh_dot_wide.h" in fatal[0] and "--arch-interaction-op dot-tril-ops" in fatal[0], r.stderr[-2000:]
        assert "[DLRM] interaction: dot-tril, 34 feature vectors, wide kernel" in r.stdout
