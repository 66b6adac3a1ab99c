#!/usr/bin/env python3
"""Strip-by-strip trace of a wedge launch (GPU): one pair on flow3's staged kernel as two chains, every strip
writing s_memrealtime (100 MHz) at its workgroup's entry, when its row codes are staged, before its first step,
after its last step and around the join.

    python tools/trace_wedge.py [N] [M]          # default 65536 65536, constants 1,-1,1,1

Prints per chain: entry to first step of strip 0, the hop lags (a strip's start behind the strip on its left,
taken from the ends: end - steps x strip 0's step), each strip's end, and the tail from the last strip's end to the
last join's end.  Times in microseconds from the earliest entry of the launch."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import concurrentproject_amd as sw
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    M = int(sys.argv[2]) if len(sys.argv) > 2 else N
    torch.cuda.set_device(0)
    sw.set_params(sw.Params(1, -1, 1, 1))
    sw.set_option("orient", 1)
    a, b = sw.gen_pair(max(N, M), max(N, M))
    a, b = a[:N], b[:M]
    arena = torch.from_numpy(np.concatenate([a, b])).cuda()
    scores = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    os.environ["SWMI_F3WEDGE_TRACE"] = "1"

    def go():
        sw.score_batch_device(arena.data_ptr(), [0], [N], [N], [M], scores.data_ptr(), flags=1, stream=s.cuda_stream)
        torch.cuda.synchronize()
        sw.stream_status(s.cuda_stream)

    for _ in range(3):
        go()
    st = sw.last_stats()
    if not st["variant"] & (1 << 18):
        sys.exit("not a wedge launch: %r" % (st,))
    # The buffer is sized from the plan the engine made: items = 2 chains x ceil(S / 4) groups, so no chain has
    # more than 2 * items strips.  A steep plan's S is a multiple of 4, exactly that many; the uniform plan's is
    # ceil((N - 2) / 126) (sw_internal.h wedge_bounds), checked against the groups.
    smax = 2 * st["items"]
    S = smax if st["variant"] & (1 << 19) else (N - 2 + 125) // 126
    if S > smax or 2 * ((S + 3) // 4) != st["items"]:
        sys.exit("the plan's %d items do not hold %d strips a chain" % (st["items"], S))
    trace = torch.zeros(16 * 2 * smax, dtype=torch.int64, device="cuda")
    sw.set_option("trace", trace.data_ptr())
    go()
    sw.set_option("trace", 0)
    t = trace.cpu().numpy()[:16 * 2 * S].reshape(2, S, 16).astype(np.int64)
    t0 = t[:, :, 0].min()
    us = lambda x: (x - t0) / 100.0
    out = {"N": N, "M": M, "score": int(scores[0].item()), "strips": S, "items": st["items"],
           "kernel_us": float(us(t[:, :, 5].max()))}
    print(json.dumps(out))
    for c in range(2):
        r = t[c]
        entry, staged, first, last, j0, j1, steps = tuple(us(r[:, k]) for k in (0, 1, 2, 3, 4, 5)) + (r[:, 8],)
        step = (last[0] - first[0]) / steps[0]
        start = last - steps * step          # where a strip's steps would start at strip 0's pace
        lag = np.diff(start)
        ing = np.array([(k + 1) % 4 != 0 for k in range(S - 1)], dtype=bool)
        print(json.dumps({
            "chain": c, "strip0_steps": int(steps[0]), "strip0_ns_per_step": round(1000 * step, 3),
            "strip0_entry_us": round(float(entry[0]), 2), "strip0_staged_us": round(float(staged[0] - entry[0]), 2),
            "strip0_prologue_us": round(float(first[0] - staged[0]), 2),
            "strip0_entry_to_first_us": round(float(first[0] - entry[0]), 2),
            "strip0_end_us": round(float(last[0]), 2), "last_end_us": round(float(last.max()), 2),
            "last_end_strip": int(last.argmax()),
            "lag_ingroup_us_median": round(float(np.median(lag[ing])), 3),
            "lag_crossgroup_us_median": round(float(np.median(lag[~ing])), 3),
            "lag_first_hops_us": [round(float(x), 2) for x in lag[:8]],
            "join_us_median": round(float(np.median(j1 - j0)), 2), "join_us_of_last_strip": round(float((j1 - j0)[last.argmax()]), 2),
            "tail_us": round(float(us(t[:, :, 5].max()) - last.max()), 2),
            "slow_polls_strip0": int(r[0, 6]),
        }))
        ks = sorted(set(range(0, 8)) | set(range(8, S, max(1, S // 16))) | set(range(S - 4, S)))
        for k in ks:
            print("chain", c, "strip", k, "steps", int(steps[k]), "entry", round(float(entry[k]), 1), "first",
                  round(float(first[k]), 1), "end", round(float(last[k]), 1), "join_end", round(float(j1[k]), 1))
    ends = us(t[:, :, 3])
    print(json.dumps({"tail_from_last_strip_end_us": round(float(us(t[:, :, 5].max()) - ends.max()), 2),
                      "last_strip": [int(x) for x in np.unravel_index(ends.argmax(), ends.shape)]}))


if __name__ == "__main__":
    main()
