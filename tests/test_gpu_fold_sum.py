"""GPU tests (-m gpu) of the wide-row segmented sum behind ffh_fold_segment_sum (csrc/fold_sum.hip) through the C ABI: tables of 1, 3, 300 and 5000 rows
in one call, 2,500 lookups per table (three 1024-blocks, the last one ragged, its last 32-block of 4 entries) as bags of 1 and 2, widths 1024 and 256,
dy read with a leading dimension above the width.  G must hold the BITS of the canonical order (include/ff_hip.h), lie within the project's bound of
float64, leave rows that are not hit at exactly 0 and the row behind the last table alone, and come out the same on a second call and on another
stream.  Width 192 is not served by the new form: the fused update's route runs, under the same assertions."""
import numpy as np
import pytest
import torch

from dlrm_flexflow_amd import capi
import fold_helpers as FH
import fold_sum_helpers as SH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7.0


@pytest.fixture(scope="module")
def fold(hip):
    return capi.fold_api(hip)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cached inputs are read-only)


def segment_sum(hip, fold, idd, dyd, width, bag, stream=None):
    """G of all tables in one call, pre-filled with a sentinel, one spare row behind the last table; the route the call took."""
    G = torch.full((sum(SH.ROWS) + 1, width), SENT, device=DEV)
    tabs, r0 = [], 0
    for t, r in enumerate(SH.ROWS):
        tabs.append((idd[t], G[r0:], dyd, r, SH.LD))
        r0 += r
    fold.call("ffh_fold_segment_sum", hip.emb_tables(tabs), len(SH.ROWS), bag, width, SH.SHAPES[bag], stream)
    route = hip.lib.ffh_embedding_last_route(hip.ctx).decode()
    torch.cuda.synchronize()
    return G.cpu().numpy(), route


def check(hip, fold, bag, width):
    """Assertions (a) to (d) of every id kind at this bag and width; the routes seen."""
    batch = SH.SHAPES[bag]
    n = hip.lib.ffh_embedding_bwd_workspace_bytes(len(SH.ROWS), bag, width, batch) + 256
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    hip.set_workspace(ws, n)
    side = torch.cuda.Stream()
    routes = set()
    for kind in SH.KINDS:
        dy, ids = SH.inputs(bag, kind)
        dyd, idd = dev(dy), [dev(i) for i in ids]
        got, route = segment_sum(hip, fold, idd, dyd, width, bag)
        routes.add(route)
        assert np.all(got[-1] == SENT), "the row behind the last table was written"
        r0 = 0
        for t, r in enumerate(SH.ROWS):
            can, ref, mass = SH.references(bag, kind)[t]
            g = got[r0:r0 + r]
            what = f"{r} rows, width {width}, bag {bag}, ids {kind}"
            diff = np.flatnonzero((g != can[:, :width]).any(1))
            print(f"segment sum, {what}: {len(diff)} rows differ from the canonical order")
            FH.assert_within(g, ref[:, :width], mass[:, :width], f"segment sum, {what}")
            assert np.array_equal(g, can[:, :width]), f"segment sum, {what}: not the canonical order in rows {diff[:8]}"
            hit = np.zeros(r, bool)
            hit[ids[t].reshape(-1)] = True
            assert not g[~hit].any(), "a row that was not hit is not exactly 0"
            r0 += r
        again, _ = segment_sum(hip, fold, idd, dyd, width, bag)
        assert again.tobytes() == got.tobytes(), "two calls differ"
        other, _ = segment_sum(hip, fold, idd, dyd, width, bag, stream=side.cuda_stream)
        assert other.tobytes() == got.tobytes(), "a call on another stream differs"
    return routes


@pytest.mark.parametrize("width", [1024, 256])
@pytest.mark.parametrize("bag", [1, 2])
def test_wide_rows_in_the_canonical_order(hip, fold, bag, width):
    routes = check(hip, fold, bag, width)
    assert all(r.startswith("fold_sum:wide|slice=") for r in routes), routes


@pytest.mark.parametrize("bag", [1, 2])
def test_a_width_the_wide_form_does_not_serve(hip, fold, bag):
    routes = check(hip, fold, bag, 192)
    assert all(r.split(":")[0] in ("small", "lsd", "buckets") for r in routes), routes
