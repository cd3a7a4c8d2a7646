"""The grid-capped streaming kernels past their caps, the part that needs no GPU (tests/stream_helpers.py; the GPU cases are
tests/test_gpu_stream_cap.py):
  * the cap table against the source text: a changed per_block or cap fails here until the shapes follow;
  * the trip count every case was written for;
  * every case's generator, reference and checker run against the CPU oracle (numpy stand-ins for the entries it does not export), and
    the checker shown to reject -- naming the first bad index -- a result whose second trip never ran and one whose second trip ran twice."""
import os
import re

import numpy as np
import pytest

import stream_helpers as S

VEC4 = ("ffh_sgd", "ffh_adam", "ffh_adagrad", "ffh_sum_slices", "ffh_concat", "ffh_convert_f32_to_bf16", "ffh_fill_f32", "ffh_cross")


@pytest.fixture(scope="module")
def host(oracle):
    return S.Backend(oracle.lib(), oracle.lib())


def host_cases():
    """every case but the mirrors of the product library's math modes (the oracle has no modes to keep them in)"""
    return [c for c in S.CASES if not c.args.get("mirror")]


# ---- 1. the caps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, r in S.TABLE.items() if not callable(r.cap)))
def test_cap_table_equals_the_source(name):
    row = S.TABLE[name]
    for work, per_block, cap in S.source_grid(row):
        assert work in S.WORK_EXPR[row.file, row.func], f"{name}: {row.file} now sizes its grid by `{work}`; restate it in the table's work function"
        assert (per_block, cap) == (row.per_block, row.cap), f"{name}: {row.file} launches ffh_grid(.., {per_block}, {cap}); the table (and its cases) say {row.per_block}, {row.cap}"


def test_gather_caps_equal_the_source():
    """the gathers take their cap from a lab switch's default and size their workgroups in rows"""
    text = open(os.path.join(S.CSRC, "embedding_fwd.hip")).read()
    body = text[text.index("int emb_fwd_launch("):text.index("int emb_fwd_bags_launch(")]
    assert re.search(r'FFH_LAB_INT\("FFH_EMB_FWD_CAP", (\d+)\)', body).group(1) == str(S.GATHER_CAP)
    assert "cap_env / nt > 0 ? cap_env / nt : 1" in body and "if (gx > cap) gx = cap;" in body
    assert re.search(r"constexpr int U = (\d+);", body).group(1) == str(S.GATHER_U)
    assert "block_rows(int U) const { return 4LL * rpw * U; }" in text and "lpr = nvec < 64 ? nvec : 64;" in text and "rpw = 64 / lpr;" in text
    assert re.search(r'FFH_LAB_INT\("FFH_EMB_BAGS_CAP", 2048\)', text)
    assert "#define FFH_LAB_INT(name, dflt) (dflt)" in open(os.path.join(S.CSRC, "ffh_common.h")).read()
    assert S.gather_block_rows({"D": 128}) == 32 and S.gather_block_rows({"D": 3}) == 4 * 21 * 4


def test_default_cap_and_workgroup_size():
    text = open(os.path.join(S.CSRC, "ffh_common.h")).read()
    assert re.search(r"ffh_grid\(int64_t work_items, int per_block, unsigned cap = 2048\)", text)
    for row in S.TABLE.values():          # every launch of the table is 256 threads wide
        src = open(os.path.join(S.CSRC, row.file)).read()
        assert "dim3(256)" in src or "dim3(kThreads)" in src


def test_every_entry_of_the_table_has_the_three_cases():
    for entry in {r.split("/")[0] for r in S.TABLE}:
        names = {c.name for c in S.CASES if c.entry == entry}
        assert names == {"at", "past", "deep"}, (entry, names)
    assert {c.entry for c in S.CASES} == {r.split("/")[0] for r in S.TABLE}
    assert set(S.RUN) == {c.entry for c in S.CASES}


def test_lab_variables_are_unset():
    assert "FFH_EMB_FWD_CAP" not in os.environ and "FFH_EMB_BAGS_CAP" not in os.environ


# ---- 2. the trip counts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_trip_count_of_the_case(c):
    t = S.assert_trips(c)
    row = S.row_of(c)
    assert t == S.trips(c.entry, c) == S.ceil_div(S.work_of(c), S.unit_of(c) * S.blocks_of(c))
    if callable(row.per_block):
        assert {"at": t == 1, "past": t == 2, "deep": t >= 3}[c.name]
    elif row.per_block == 256:
        assert S.unit_of(c) == 256
        assert {"at": t == 1, "past": t == 2, "deep": t >= 3}[c.name]
        if c.name == "at":
            assert S.work_of(c) == 256 * S.blocks_of(c)


def test_the_shapes_the_cases_were_written_for():
    by = {(c.entry, c.name, tuple(sorted(c.args.items()))): c for c in S.CASES}
    past = next(c for c in S.CASES if c.entry == "ffh_cross_fwd" and c.name == "past")
    groups, stride = past.args["dim"] // 4, 256 * 2048
    assert S.work_of(past) == 524448 and (stride // groups, stride % groups) == (606, 704) and groups - 704 == 160
    # in that case only threads that then leave the batch carry; in the 99-group one the second trip's threads 16 .. 114 carry into the last row
    short = next(c for c in S.CASES if c.entry == "ffh_cross_fwd" and c.args["batch"] == 5297)
    g2 = short.args["dim"] // 4
    assert (stride // g2, stride % g2) == (5295, 83) and S.work_of(short) - stride == 115 and 0 + 5295 + 1 == short.args["batch"] - 1
    long_row = next(c for c in S.CASES if c.entry == "ffh_cross_fwd" and c.args["batch"] == 2)
    assert stride // (long_row.args["dim"] // 4) == 0
    concat = next(c for c in S.CASES if c.entry == "ffh_concat_fwd" and c.name == "past")
    assert S.work_of(concat) == 264321 and 513 % 4 == 1
    tril = next(c for c in S.CASES if c.entry == "ffh_tril_fwd" and c.name == "past")
    assert S.work_of(tril) == 4195296
    assert len(by) == len(S.CASES)


# ---- 3. the checker proof ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", host_cases(), ids=S.case_id)
def test_case_runs_clean_against_the_oracle(host, c):
    host.tamper = None
    worst = S.run_case(host, c)
    assert worst <= 1.0


def tamper_cases():
    """the `past` cases of every entry whose call leaves an array of at least its work's size behind (not the counters and sums of the
    metrics and the digest, nor the 1000-row table the dense embedding backward adds 8257 rows into)"""
    return [c for c in host_cases() if c.name == "past" and c.entry not in ("ffh_metrics_update", "ffh_ctr_eval_update", "ffh_state_digest",
                                                                            "ffh_embedding_bwd_dense", "ffh_init_uniform_bf16")]


@pytest.mark.parametrize("mode", ["stale", "twice"])
@pytest.mark.parametrize("c", tamper_cases(), ids=S.case_id)
def test_checker_rejects_the_wrong_result_and_names_the_first_bad_index(host, c, mode):
    vec = 4 if c.entry.startswith(VEC4) and not (c.args.get("scalar") or c.args.get("row")) and c.args.get("vec", True) else 1
    host.tamper = S.Tamper(mode, 256 * S.blocks_of(c) * vec)
    try:
        with pytest.raises(AssertionError) as e:
            S.run_case(host, c)
    finally:
        planted, host.tamper = host.tamper.first, None
    assert planted, "nothing was planted"
    m = re.match(r"(.+?)( \(.*?\))?: \d+ of \d+ elements (differ|past the bound), first bad index (\d+)", str(e.value))
    assert m, str(e.value)
    name = m.group(1)
    assert name in planted and int(m.group(4)) == planted[name], (str(e.value)[:200], planted)


def test_checker_on_small_arrays():
    a = np.arange(8, dtype=np.float32)
    assert S.check("a", a, a.copy()) == 0.0
    b = a.copy(); b[5] = np.nextafter(b[5], np.float32(9))
    with pytest.raises(AssertionError, match="first bad index 5"):
        S.check("a", b, a)
    s = S.sentinels(np.float32, 4)
    t = s.copy(); t[2] = np.float32(np.nan)          # another NaN in a sentinel's place is a write
    with pytest.raises(AssertionError, match="first bad index 2"):
        S.check("s", t, s)
    n1, n2 = np.array([np.nan], np.float32), np.array([0xFFC00000], np.uint32).view(np.float32)
    S.check("nan", n1, n2)                           # NaNs the arithmetic made: the payload is not compared
    with pytest.raises(AssertionError, match="first bad index 3"):
        S.check_close("c", a + np.float32([0, 0, 0, 1, 0, 0, 0, 1]), a.astype(np.float64), 0.5)
    assert S.check_close("c", a, a.astype(np.float64) + 0.25, 0.5) == 0.5
