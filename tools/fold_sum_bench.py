"""ffh_fold_segment_sum alone at the flagship shape: the 13 folded Terabyte tables, width 1024, batch 32768, uniform ids.  Prints the route and the time of
one call (memset of G + sort + sum) over `rounds` rounds of `iters` back-to-back calls, against the bytes the sum has to move (13 x 32768 rows of dy read,
G written).  FFH_TOOLS_LIB=<libffhip.so of another build> measures that build (tools/_lab.py).
    python tools/fold_sum_bench.py [rounds] [iters]"""
import sys

import numpy as np
import torch

import _lab
from dlrm_flexflow_amd import capi

ROWS = [7420, 3, 7120, 1543, 63, 10, 2208, 155, 4, 976, 14, 108, 36]
WIDTH, BATCH = 1024, 32768


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    hip = _lab.load_hip(0)
    fold = capi.fold_api(hip)
    rng = np.random.default_rng(1)
    dy = torch.from_numpy(rng.uniform(-1, 1, (BATCH, WIDTH)).astype(np.float32)).cuda()
    ids = [torch.from_numpy(rng.integers(0, r, (BATCH, 1)).astype(np.int64)).cuda() for r in ROWS]
    G = torch.empty(sum(ROWS), WIDTH, device="cuda")
    n = hip.lib.ffh_embedding_bwd_workspace_bytes(len(ROWS), 1, WIDTH, BATCH) + 256
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    hip.set_workspace(ws, n)
    tabs, r0 = [], 0
    for t, r in enumerate(ROWS):
        tabs.append((ids[t], G[r0:], dy, r, WIDTH))
        r0 += r
    tabs = hip.emb_tables(tabs)

    def call():
        fold.call("ffh_fold_segment_sum", tabs, len(ROWS), 1, WIDTH, BATCH, None)
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    route = hip.lib.ffh_embedding_last_route(hip.ctx).decode()
    us = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / iters * 1e3)
    gb = (len(ROWS) * BATCH * WIDTH * 4 + sum(ROWS) * WIDTH * 4) / 1e9
    med = float(np.median(us))
    print(f"fold_segment_sum route {route}: median {med:.1f} us  min {min(us):.1f}  max {max(us):.1f}  ({rounds} rounds of {iters} calls); "
          f"{gb:.2f} GB read + written: {gb / med * 1e3:.2f} TB/s;  checksum {float(G.double().abs().sum()):.6e}", flush=True)


if __name__ == "__main__":
    main()
