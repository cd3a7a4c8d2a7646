"""CPU tests of checkpoint save / exact resume (no GPU is opened): the numpy restatement of the digest
(ffmodel.state_digest_reference) against a plain-Python restatement and the header's own inline function; the symbol list against the
libraries and the bindings; and the driver with the CPU oracle as kernel library -- exact resume for every optimizer and table-optimizer
placement, the flags, every refusal of load, two gloo ranks, and the unchanged output of a run without the new flags.

The CPU oracle exports neither the CTR nor the data extension, so a run on it can neither evaluate (--eval-batches) nor shuffle
(--data-randomize total): those parts of the resume check (EVAL lines, --eval-only, the shuffle order) run on the HIP library in
tests/test_gpu_checkpoint.py; here the run walks its batches in file order (--synthetic-labels logistic) and the checkpoints are compared."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dlrm_flexflow_amd import build, capi, ffmodel
import checkpoint_helpers as K

HOST_LIB = os.path.join(ROOT, "dlrm_flexflow_amd", "host", "libffmodel.so")
RUN_DLRM = os.path.join(ROOT, "dlrm_flexflow_amd", "run_dlrm.py")
M64 = 2 ** 64 - 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


@pytest.fixture(scope="module")
def backend():
    import dlrm_helpers as H
    return H.oracle_backend()


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------
def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def plain_digest(rows, seed, index_base=0):
    """the definition of include/ff_hip_digest.h in Python integers; rows: a list of bytes objects of one length"""
    W = (len(rows[0]) + 7) // 8
    total = 0
    for r, row in enumerate(rows):
        for w in range(W):
            word = int.from_bytes(row[8 * w:8 * w + 8], "little")            # a short slice reads as zero-extended
            i = (index_base + r * W + w) & M64
            total += _mix(_mix((_mix(seed) + i) & M64) ^ word)
    return total & M64


@pytest.mark.parametrize("rows,rb", [(1, 2), (3, 6), (5, 8), (4, 26), (7, 52), (2, 72)])
@pytest.mark.parametrize("index_base", [0, 2 ** 32 - 5, 2 ** 40, 2 ** 64 - 3])
def test_reference_equals_the_plain_python_restatement_and_the_header(rows, rb, index_base):
    raw = np.random.default_rng(rows * 100 + rb).integers(0, 256, (rows, rb), dtype=np.uint8)
    exp = plain_digest([bytes(r) for r in raw], 0xABCDEF12345, index_base)
    assert ffmodel.state_digest_reference(raw, 0xABCDEF12345, index_base) == exp
    assert ffmodel.state_digest_reference(raw.tobytes(), 0xABCDEF12345, index_base, row_bytes=rb) == exp
    assert ffmodel.state_digest_host(raw, 0xABCDEF12345, index_base, row_bytes=rb) == exp        # ffh_state_digest_host as the host layer compiles it


def test_reference_does_not_depend_on_the_leading_dimension():
    rng = np.random.default_rng(1)
    logical = rng.standard_normal((9, 13)).astype(np.float32)
    wide = np.full((9, 32), np.float32(-7.25e9))
    wide[:, :13] = logical
    assert ffmodel.state_digest_reference(wide[:, :13], 5) == ffmodel.state_digest_reference(logical, 5)
    # the header's function on the padded buffer itself: rows 128 bytes apart, 52 of them counted
    assert ffmodel.state_digest_host(wide.astype(np.float32)[:, :32], 5, row_bytes=52, ld_bytes=128) == ffmodel.state_digest_reference(logical, 5)
    wide[:, 13:] = 1.0
    assert ffmodel.state_digest_host(wide.astype(np.float32), 5, row_bytes=52, ld_bytes=128) == ffmodel.state_digest_reference(logical, 5)


def test_reference_sees_a_swap_and_a_flipped_bit():
    a = np.arange(64, dtype=np.uint64).reshape(4, 16)
    d = ffmodel.state_digest_reference(a, 3)
    b = a.copy()
    b[0, 1], b[2, 5] = a[2, 5], a[0, 1]                      # two unequal words change places
    assert ffmodel.state_digest_reference(b, 3) != d
    for bit in (0, 17, 63):
        c = a.copy()
        c[3, 15] ^= np.uint64(1 << bit)
        assert ffmodel.state_digest_reference(c, 3) != d
    assert ffmodel.state_digest_reference(a, 4) != d          # another seed, another word
    assert ffmodel.state_digest_reference(a[:0], 3) == 0


@pytest.mark.parametrize("rb", [6, 8, 26, 72])
def test_index_base_splits_compose(rb):
    raw = np.random.default_rng(rb).integers(0, 256, (11, rb), dtype=np.uint8)
    W = (rb + 7) // 8
    whole = ffmodel.state_digest_reference(raw, 21, 2 ** 32 - 5)
    for a in (0, 1, 4, 11):
        parts = ffmodel.state_digest_reference(raw[:a], 21, 2 ** 32 - 5) + ffmodel.state_digest_reference(raw[a:], 21, 2 ** 32 - 5 + a * W)
        assert parts & M64 == whole


# ---- 2. the header's list, the libraries, the bindings ---------------------------------------------------------------------------------
def test_digest_header_list_declarations_and_prototypes_agree():
    syms = capi.digest_header_symbols()
    assert syms == ["ffh_digest_abi_version", "ffh_state_digest"]
    assert set(syms) == set(capi._SIGS_DIGEST)
    text = open(capi.DIGEST_HEADER_PATH).read()
    body = text.split("#define FFH_DIGEST_API_LIST")[0]
    declared = set(re.findall(r"^int\s+(ffh_[a-z0-9_]+)\s*\(", body, re.M))
    assert declared == set(syms), declared ^ set(syms)
    assert capi.digest_header_abi_version() == 1
    # include/ff_hip.h: list and ABI version untouched by the extension
    assert not set(syms) & set(capi.header_symbols())
    assert set(capi.header_symbols()) == set(capi._SIGS)
    assert capi.header_abi_version() == 14
    params = re.search(r"^int\s+ffh_state_digest\s*\((.*?)\);", body, re.M | re.S).group(1)
    assert len(params.split(",")) == len(capi._SIGS_DIGEST["ffh_state_digest"][1])


def test_hip_library_exports_the_extension_and_the_oracle_does_not(oracle):
    exp = _exported(build.build_hip())
    assert set(capi.digest_header_symbols()) <= exp
    assert not set(capi.digest_header_symbols()) & _exported(oracle.ORACLE_LIB)
    with pytest.raises(capi.FFHError, match="no digest extension"):
        capi.digest_api(oracle.lib())


def test_c_api_and_python_face_export_the_entries():
    assert {"flexflow_model_save_checkpoint", "flexflow_model_load_checkpoint", "flexflow_model_state_digest"} <= _exported(HOST_LIB)
    for name in ("save_checkpoint", "load_checkpoint", "state_digest"):
        assert callable(getattr(ffmodel.FFModel, name))
    assert callable(ffmodel.read_checkpoint) and callable(ffmodel.state_digest_reference)


# ---- 3. exact resume ---------------------------------------------------------------------------------------------------------------------
OPTIMIZERS = {
    "sgd": ["--optimizer", "sgd"],
    "sgd-momentum": ["--optimizer", "sgd-momentum"],
    "adam-dense-tables": ["--optimizer", "adam"],
    "adam-sparse-tables": ["--optimizer", "adam", "--sparse-embedding-optimizer"],
    "sgd-momentum-sparse-tables": ["--optimizer", "sgd-momentum", "--sparse-embedding-optimizer"],
}


@pytest.mark.parametrize("opt", sorted(OPTIMIZERS))
def test_resume_is_bit_exact(backend, tmp_path, opt):
    """4 epochs straight (A) against 2 epochs, save (B), a NEW process that loads B and trains to 4 (C), with a schedule whose warm-up and decay
    both lie inside the run: A and C agree record by record, bit for bit, and in every run field and digest -- parameters, optimizer state,
    Adam's scalars, the step count the host-route schedule stands at."""
    flags = K.MODEL + K.SCHEDULE + OPTIMIZERS[opt]
    (ra, rb, rc), (a, b, c) = K.abc(backend, tmp_path, flags)
    ck = K.assert_same_checkpoint(os.path.join(a, "rank-0-of-1.ffck"), os.path.join(c, "rank-0-of-1.ffck"))
    K.assert_digests_hold(os.path.join(c, "rank-0-of-1.ffck"))
    meta = ck["meta"]
    assert meta["epochs_done"] == 4 and meta["steps"] == 17 and meta["lr_route"] == "host" and meta["lr_host_steps"] == 17      # warm-up step + 4 x 4
    assert meta["optimizer"] == OPTIMIZERS[opt][1]
    assert meta["table_optimizer"] == ("sparse" if "sparse" in opt else ("fused-sgd" if opt == "sgd" else "dense"))
    names = set(meta["records"])
    assert ("adam_scalars" in names) == opt.startswith("adam")
    assert any(n.startswith("sparse_state0/") for n in names) == ("sparse" in opt)
    assert any(n.startswith("sgd_v/Dense") for n in names) == opt.startswith("sgd-momentum")
    # the B checkpoint differs from A (training moved the state), and the resumed run says where it started
    assert ffmodel.read_checkpoint(b)["meta"]["digest"] != meta["digest"]
    assert f"[DLRM] checkpoint: loaded {b} (epoch 2, step 9, digest 0x{ffmodel.read_checkpoint(b)['meta']['digest']:016x})" in rc.stdout
    assert "[DLRM] checkpoint: none" in ra.stdout and "[DLRM] checkpoint: none" in rb.stdout
    # the training metrics of the last epoch are the straight run's; the THROUGHPUT line counts the epochs that ran
    assert ra.stderr.splitlines()[-1] == rc.stderr.splitlines()[-1] and ra.stderr.splitlines()[-1].startswith("[Metrics]")
    assert "[resumed: epochs 2 to 4]" in rc.stdout and "of checkpoint saving]" in rc.stdout
    assert "[DLRM] Num. epochs = 4" in rc.stdout


def test_checkpoint_every_epochs_leaves_the_last_file_and_no_temporary(backend, tmp_path):
    d = os.path.join(str(tmp_path), "ck")
    flags = K.MODEL + ["--optimizer", "sgd"]
    K.run_driver(backend, *flags, "--epochs", "3", "--save-checkpoint", d, "--checkpoint-every-epochs=1")
    assert os.listdir(d) == ["rank-0-of-1.ffck"]
    every = ffmodel.read_checkpoint(d)
    assert every["meta"]["epochs_done"] == 3 and every["meta"]["steps"] == 13
    e = os.path.join(str(tmp_path), "end")
    K.run_driver(backend, *flags, "--epochs", "3", "--save-checkpoint", e)
    K.assert_same_checkpoint(os.path.join(d, "rank-0-of-1.ffck"), os.path.join(e, "rank-0-of-1.ffck"))
    # a save every 2nd epoch of 3 and none at the end would have left epoch 2's: the last epoch always saves
    r = K.run_driver(backend, *flags, "--epochs", "3", "--checkpoint-every-epochs", "1", check=False)
    assert r.returncode != 0 and "--checkpoint-every-epochs 1: needs --save-checkpoint DIR" in r.stderr


def test_python_face_saves_loads_and_digests(backend, tmp_path):
    """FFModel.save_checkpoint / load_checkpoint / state_digest through the C API: a second model of another seed takes the first one's state."""
    d = os.path.join(str(tmp_path), "ck")
    flags = ["--backend", backend] + K.MODEL + ["--optimizer", "sgd-momentum"]
    a = ffmodel.DLRM(flags + ["--seed", "3"])
    a.warmup()
    a.model.save_checkpoint(d, epochs_done=7)
    da = a.model.state_digest()
    a.close()
    ck = K.assert_digests_hold(os.path.join(d, "rank-0-of-1.ffck"))
    assert ck["meta"]["digest"] == da and ck["meta"]["epochs_done"] == 7 and ck["meta"]["steps"] == 1
    b = ffmodel.DLRM(flags + ["--seed", "4"])
    assert b.model.state_digest() != da
    assert b.model.load_checkpoint(d) == {"epochs_done": 7}
    assert b.model.state_digest() == da
    b.close()


def test_run_dlrm_passes_the_flags_through(backend, tmp_path):
    d = os.path.join(str(tmp_path), "ck")
    args = ["--backend", backend] + K.MODEL + ["--optimizer", "sgd", "--epochs", "1"]
    r = subprocess.run([sys.executable, RUN_DLRM, *args, f"--save-checkpoint={d}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[DLRM] checkpoint: none" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    r = subprocess.run([sys.executable, RUN_DLRM, *args, "--load-checkpoint", d, "--epochs", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"[DLRM] checkpoint: loaded {d} (epoch 1, step 5, " in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


# ---- 4. refusals: one per bullet of DESIGN section 15's list ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def saved(backend, tmp_path_factory):
    """one 1-epoch checkpoint of the tiny model (momentum SGD), saved once; tests copy it before they damage it"""
    d = str(tmp_path_factory.mktemp("saved") / "ck")
    flags = K.MODEL + ["--optimizer", "sgd-momentum"]
    K.run_driver(backend, *flags, "--epochs", "1", "--save-checkpoint", d)
    return d, flags


def _copy(saved_dir, tmp_path):
    import shutil
    d = os.path.join(str(tmp_path), "ck")
    shutil.copytree(saved_dir, d)
    return d, os.path.join(d, "rank-0-of-1.ffck")


def _refused(backend, flags, d, *more):
    r = K.run_driver(backend, *flags, *more, "--epochs", "2", "--load-checkpoint", d, check=False)
    assert r.returncode != 0 and "THROUGHPUT" not in r.stdout, r.stdout[-1500:]
    fatal = [l for l in r.stderr.splitlines() if l.startswith("FATAL:")]
    assert len(fatal) == 1 and fatal[0].startswith(f"FATAL: --load-checkpoint {d}: "), r.stderr[-2000:]
    return fatal[0]


def _patch_manifest(path, old, new):
    assert len(old) == len(new)
    raw = bytearray(open(path, "rb").read())
    length = int.from_bytes(raw[16:24], "little")
    k = raw.find(old.encode(), 24, 24 + length)
    assert k >= 0, old
    raw[k:k + len(old)] = new.encode()
    open(path, "wb").write(raw)


def test_load_works_before_it_is_refused(backend, saved, tmp_path):
    d, flags = saved
    r = K.run_driver(backend, *flags, "--epochs", "2", "--load-checkpoint", d)
    assert "[DLRM] checkpoint: loaded" in r.stdout and "[resumed: epochs 1 to 2]" in r.stdout


def test_missing_file_is_refused(backend, saved, tmp_path):
    _, flags = saved
    msg = _refused(backend, flags, os.path.join(str(tmp_path), "nothing"))
    assert "cannot open" in msg and "rank-0-of-1.ffck" in msg and "--save-checkpoint" in msg


def test_truncated_file_is_refused(backend, saved, tmp_path):
    d, path = _copy(saved[0], tmp_path)
    size = os.path.getsize(path)
    os.truncate(path, size - 300)
    assert "is truncated (record " in _refused(backend, saved[1], d)
    os.truncate(path, 100)
    assert "is truncated (its manifest is cut short)" in _refused(backend, saved[1], d)
    os.truncate(path, 10)
    assert "is truncated (shorter than its header)" in _refused(backend, saved[1], d)


def test_wrong_magic_and_unknown_version_are_refused(backend, saved, tmp_path):
    d, path = _copy(saved[0], tmp_path)
    raw = bytearray(open(path, "rb").read())
    raw[8] = 9
    open(path, "wb").write(raw)
    assert "format version 9, this build reads version 1" in _refused(backend, saved[1], d)
    raw[0] = ord("X")
    open(path, "wb").write(raw)
    assert "is not a checkpoint file (wrong magic)" in _refused(backend, saved[1], d)


def test_a_record_the_model_lacks_and_a_parameter_the_file_lacks_are_refused(backend, saved, tmp_path):
    d, flags = saved
    deeper = [f if f != "20-8-1" else "20-8-1-1" for f in flags]
    msg = _refused(backend, deeper, d)                                # a fourth top layer: the model has a parameter the file lacks
    assert "the model has param/Dense_109/0" in msg and "has no such record" in msg and "--arch-mlp-top" in msg
    dd = os.path.join(str(tmp_path), "deeper")
    K.run_driver(backend, *deeper, "--epochs", "1", "--save-checkpoint", dd)
    msg = _refused(backend, flags, dd)                                # the other way round: the file has a record the model lacks
    assert "has record param/Dense_109/0" in msg and "the model has no such state" in msg and "--arch-mlp-top" in msg


def test_shape_and_element_type_mismatches_are_refused(backend, saved, tmp_path):
    d, flags = saved
    wider = [f if f != "20-8-1" else "20-16-1" for f in flags]
    msg = _refused(backend, wider, d)
    assert "record param/Dense_107/0 is [8][20], the model's is [16][20]" in msg and "--arch-mlp-top" in msg
    d2, path = _copy(d, tmp_path)
    _patch_manifest(path, "param/Embedding_103/0 f32", "param/Embedding_103/0 u64")
    assert "record param/Embedding_103/0 holds u64 elements, the model's are f32" in _refused(backend, flags, d2)
    _patch_manifest(path, "param/Embedding_103/0 u64", "param/Embedding_103/0 f32")
    _patch_manifest(path, "embedding_dtype fp32", "embedding_dtype bf16")
    msg = _refused(backend, flags, d2)
    assert "it holds bf16 tables, this run has --embedding-dtype fp32" in msg and "use --embedding-dtype bf16" in msg


def test_another_optimizer_and_another_table_optimizer_are_refused(backend, saved):
    d, flags = saved
    other = [f if f != "sgd-momentum" else "adam" for f in flags]
    msg = _refused(backend, other, d)
    assert "saved with --optimizer sgd-momentum, this run has --optimizer adam" in msg and "use --optimizer sgd-momentum" in msg
    msg = _refused(backend, flags, d, "--sparse-embedding-optimizer")
    assert "updated by the dense table optimizer, this run's by the sparse one" in msg and "drop --sparse-embedding-optimizer" in msg


def test_another_placement_is_refused(backend, saved, tmp_path):
    d2, path = _copy(saved[0], tmp_path)
    _patch_manifest(path, "table Embedding_104 table-wise:0", "table Embedding_104 table-wise:1")
    msg = _refused(backend, saved[1], d2)
    assert "table Embedding_104 was placed table-wise:1 when it was saved and is placed table-wise:0 now" in msg and "--row-shard-rows" in msg


@pytest.mark.parametrize("record", ["param/Dense_100/0", "sgd_v/Embedding_105/0"])
def test_a_flipped_byte_is_refused_and_the_record_is_named(backend, saved, tmp_path, record):
    d2, path = _copy(saved[0], tmp_path)
    ck = ffmodel.read_checkpoint(path)
    data_start = (24 + int.from_bytes(open(path, "rb").read(24)[16:24], "little") + 4095) // 4096 * 4096
    raw = bytearray(open(path, "rb").read())
    raw[data_start + ck["meta"]["records"][record]["offset"] + 3] ^= 0x01
    del ck
    open(path, "wb").write(raw)
    msg = _refused(backend, saved[1], d2)
    assert f"record {record} does not match its digest after the copy" in msg and "is damaged" in msg


# ---- 5. without the new flags nothing changes ----------------------------------------------------------------------------------------------
def test_output_without_the_flags_is_the_parent_commits(backend):
    """tests/golden/checkpoint_parent_transcript.txt: stdout and stderr of this very command on the commit before checkpoints existed, the
    elapsed time, the rate and the library's path replaced by placeholders."""
    r = K.run_driver(backend, *K.MODEL, *K.SCHEDULE, "--optimizer", "adam", "--epochs", "3")

    def norm(s):
        s = re.sub(r"ELAPSED TIME = [0-9.]+s, THROUGHPUT = [0-9.]+ samples/s", "ELAPSED TIME = <t>s, THROUGHPUT = <r> samples/s", s)
        return re.sub(r"\[kernel library: oracle-cpu, [^\]]*\]", "[kernel library: oracle-cpu, <path>]", s)
    golden = open(os.path.join(ROOT, "tests", "golden", "checkpoint_parent_transcript.txt")).read()
    assert "# stdout\n" + norm(r.stdout) + "# stderr\n" + norm(r.stderr) == golden


# ---- 6. two gloo ranks ---------------------------------------------------------------------------------------------------------------------
def _two_ranks(tmp_path, mode, ckdir, *more, port_offset=0):
    worker = os.path.join(ROOT, "tests", "_dist_worker_checkpoint.py")
    port = str(32100 + os.getpid() % 1500 + (1 if mode == "load" else 0) + port_offset)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, worker, "cpu", mode, str(tmp_path), ckdir, *more], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [np.load(os.path.join(str(tmp_path), f"{mode}-rank{r}.npz")) for r in range(2)]


def test_two_gloo_ranks_round_trip_and_one_rank_is_refused(backend, tmp_path):
    ckdir = os.path.join(str(tmp_path), "ck")
    saved2 = _two_ranks(tmp_path, "save", ckdir)
    assert sorted(os.listdir(ckdir)) == ["rank-0-of-2.ffck", "rank-1-of-2.ffck"]
    loaded = _two_ranks(tmp_path, "load", ckdir)
    tables = set()
    for r in range(2):
        ck = K.assert_digests_hold(os.path.join(ckdir, f"rank-{r}-of-2.ffck"))
        assert ck["meta"]["world_size"] == 2 and ck["meta"]["rank"] == r and ck["meta"]["epochs_done"] == 1
        assert int(saved2[r]["digest"]) == int(loaded[r]["digest"]) == ck["meta"]["digest"]
        assert int(loaded[r]["epochs_done"]) == 1
        mine = {n for n in ck["meta"]["records"] if n.startswith("param/Embedding")}
        assert len(mine) == 2 and not mine & tables                  # table-wise: each rank holds and saves its own two tables
        tables |= mine
        assert {t: p for t, p in ck["meta"]["tables"].items()} == {f"Embedding_{102 + t}": f"table-wise:{t % 2}" for t in range(4)}
    msg = _refused(backend, K.MODEL + ["--optimizer", "sgd-momentum"], ckdir)
    assert "it was saved by 2 ranks and this run has 1" in msg and "launch 2 ranks" in msg


PLACEMENTS = {                                   # the tables have 30, 20, 10 and 40 rows of 4 columns
    "row": (["--row-shard-rows", "35"], "Embedding_105", ["row:0:20", "row:20:20"]),
    "column": (["--column-shard-rows", "35"], "Embedding_105", ["column:0:2", "column:2:2"]),
    "replicated": (["--replicate-embedding-rows", "15"], "Embedding_104", ["replicated", "replicated"]),
}


@pytest.mark.parametrize("placement", sorted(PLACEMENTS))
def test_two_gloo_ranks_resume_exactly_with_a_sharded_or_replicated_table(backend, tmp_path, placement):
    """Row shard (its spare zero row is not saved and is cleared on load), column shard and replicated table: 2 epochs straight (A) against 1 epoch,
    save (B), two new ranks that load B and train to 2 (C).  Every rank's A and C files agree record by record; the manifest names the placement and
    the record has the slice's shape; the same directory is refused under table-wise placement."""
    more, table, placed = PLACEMENTS[placement]
    dirs = {}
    for k, name in enumerate("ABC"):
        dirs[name] = os.path.join(str(tmp_path), name)
        os.mkdir(os.path.join(str(tmp_path), "out" + name))
    out = {n: os.path.join(str(tmp_path), "out" + n) for n in "ABC"}
    _two_ranks(out["A"], "save", dirs["A"], *more, "--epochs", "2", port_offset=2)
    _two_ranks(out["B"], "save", dirs["B"], *more, port_offset=4)
    loaded = _two_ranks(out["C"], "load", dirs["B"], *more, "--epochs", "2", "--save-checkpoint", dirs["C"], port_offset=6)
    shape = {"row": (20, 4), "column": (40, 2), "replicated": (10, 4)}[placement]
    for r in range(2):
        f = f"rank-{r}-of-2.ffck"
        ck = K.assert_same_checkpoint(os.path.join(dirs["A"], f), os.path.join(dirs["C"], f))
        K.assert_digests_hold(os.path.join(dirs["C"], f))
        assert ck["meta"]["tables"][table] == placed[r] and ck["meta"]["epochs_done"] == 2
        assert ck[f"param/{table}/0"].shape == shape and ck[f"sgd_v/{table}/0"].shape == shape
        assert int(loaded[r]["digest"]) == ck["meta"]["digest"] and int(loaded[r]["epochs_done"]) == 1
    if placement == "replicated":
        a0, a1 = (ffmodel.read_checkpoint(os.path.join(dirs["C"], f"rank-{r}-of-2.ffck")) for r in range(2))
        assert a0[f"param/{table}/0"].tobytes() == a1[f"param/{table}/0"].tobytes()
