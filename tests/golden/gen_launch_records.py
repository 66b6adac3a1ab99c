"""Records what the engine decides for a fixed list of calls (tests/golden/launch_records.json): for
each case its inputs, the planning fields of sw_last_stats (mode, W, C, dna, blocks, waves_per_cu,
items, variant, boundary_bytes, cells) and the score, checked against the CPU oracle as it is
recorded.  tests/test_launch_records.py replays the file: a host-side change that makes one of these
calls launch something else fails there.  Kernel times are not recorded.

The cases take the option sets of the tests that force each path (test_flow3*.py, test_hepta.py,
test_ring*.py, test_pwg*.py, test_duo_*.py, test_slab.py) at small shapes, one launch each.  Between
them they reach every mode 0..5, each variant bit 0..17 set and clear, and each of the 29 flow3
kernels (coverage_missing).  The decisions depend on the CU count, which the file states.

    python tests/golden/gen_launch_records.py [out.json]     # on the MI355X; default: rewrites the JSON
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "launch_records.json")
FIELDS = ("mode", "W", "C", "dna", "blocks", "waves_per_cu", "items", "variant", "boundary_bytes", "cells")

# every option's default (include/algoGPU.h): a case starts from these
DEFAULTS = {
    "W": 0, "C": 0, "bytes": 0, "duo16": 1, "f2stream": 0, "f3pwg": 1, "timeout": 30, "blocks": 0,
    "stall_item": -1, "trace": 0, "trace_mb": 1024, "orient": 0, "mode": -1, "f2_wgs": 0, "f2w": 0,
    "f2pwg": -1, "ring": -1, "f3split": -1, "linear": -1, "f3": 1, "f3a": 1, "f3hl": 1, "f3slab": 1,
    "duo_lds": 1, "duo_roles": 1, "duo_raw": 1, "hep": 1, "f3rhl": 0, "f3pool": 0, "slab_plain": 0,
    "duo_tab": 1, "duo_prio": -1, "ring_rows": 4096,
}

LIN, AFF = (1, -1, 1, 1), (2, -3, 5, 2)
RING = {"ring": 1, "ring_rows": 512, "blocks": 2}
SLAB = {"ring_rows": 512, "blocks": 2, "slab_plain": 1}


def _case(name, kind, params, opts, n, m, pairs=1, alphabet="dna"):
    return {"name": name, "kind": kind, "params": list(params), "options": dict(opts), "n": n, "m": m,
            "pairs": pairs, "alphabet": alphabet}


def cases():
    """kind: "pair" = one host pair (seq1 across the lanes), "device" = the same through
    sw_score_batch_device (alphabet scanned on the device), "slab" = one column slab without edges,
    "batch" = `pairs` host pairs of n + (k mod 50) by m bytes."""
    cs = []
    one = {"orient": 1}
    # flow3's staged kernels: a pair of 700 x 500 (six two-column strips in two groups)
    staged = (("lin_c32hl", LIN, {}), ("lin_c32", LIN, {"f3hl": 0, "C": 32}), ("lin_c16", LIN, {"f3hl": 0}),
              ("aff_c32hl", AFF, {}), ("aff_c32", AFF, {"f3hl": 0}), ("aff_c16", AFF, {"C": 16}))
    for alphabet in ("dna", "lower"):
        for name, prm, o in staged:
            cs.append(_case("staged_%s_%s" % (name, alphabet), "pair", prm, {**one, **o}, 700, 500, alphabet=alphabet))
    cs.append(_case("staged_lin_pool", "pair", LIN, {**one, "f3pool": 1}, 700, 500))
    cs.append(_case("staged_aff_pool", "pair", AFF, {**one, "f3pool": 1}, 700, 500))
    cs.append(_case("staged_lin_cut", "pair", LIN, {**one, "f3split": 1}, 700, 500))
    cs.append(_case("staged_lower_device", "device", LIN, dict(one), 700, 500, alphabet="lower"))
    cs.append(_case("flow2_staged_lin", "pair", LIN, {**one, "f3": 0}, 700, 500))
    cs.append(_case("flow2_staged_aff", "pair", AFF, {**one, "f3a": 0}, 700, 500))
    cs.append(_case("flow2_streamed_lin", "pair", LIN, {**one, "f2stream": 1}, 700, 500))
    # ring mode on two blocks with 512-row rings
    ring = {**one, **RING}
    cs.append(_case("ring_lin_c64", "pair", LIN, {**ring, "f2w": 2}, 1100, 700))
    cs.append(_case("ring_lin_c64hl", "pair", LIN, {**ring, "f2w": 2, "f3rhl": 1}, 1100, 700))
    cs.append(_case("ring_lin_c32", "pair", LIN, {**ring, "f2w": 2, "C": 32}, 1100, 700))
    cs.append(_case("ring_aff", "pair", AFF, {**ring, "f2w": 2}, 1100, 700))
    cs.append(_case("ring_lin_w3", "pair", LIN, ring, 1500, 700))
    cs.append(_case("ring_aff_w3", "pair", AFF, ring, 1500, 700))
    cs.append(_case("ring_lin_w3_lower", "pair", LIN, ring, 1500, 700, alphabet="lower"))
    cs.append(_case("ring_aff_w3_lower", "pair", AFF, ring, 1500, 700, alphabet="lower"))
    for n, m, blocks in ((1100, 700, 1), (2000, 1000, 2), (2400, 600, 3)):
        cs.append(_case("ring_w45_b%d" % blocks, "pair", LIN, {**ring, "f2w": 4, "blocks": blocks}, n, m))
    cs.append(_case("flow2_ring_lin", "pair", LIN, {**ring, "f2w": 2, "f3": 0}, 1100, 700))
    # single-GPU column slabs (no edges)
    cs.append(_case("slab_lin", "slab", LIN, {**SLAB, "f2w": 2}, 1100, 700))
    cs.append(_case("slab_aff", "slab", AFF, {**SLAB, "f2w": 2}, 1100, 700))
    cs.append(_case("slab_lin_w3", "slab", LIN, SLAB, 1500, 700))
    cs.append(_case("slab_aff_w3", "slab", AFF, SLAB, 1500, 700))
    cs.append(_case("flow2_slab", "slab", LIN, {**SLAB, "f3slab": 0}, 1100, 700))
    # the other grid organisations
    cs.append(_case("strip_batch", "batch", LIN, {}, 300, 300, pairs=8))
    cs.append(_case("pairwg_batch", "batch", LIN, {"mode": 1}, 400, 450, pairs=8))
    cs.append(_case("chain_pair", "pair", AFF, {**one, "mode": 2}, 700, 500))
    cs.append(_case("flow_pair", "pair", (2, -3, 130, 2), dict(one), 700, 500))
    # batches: fewer pairs than CUs (item claim), fewer than two per CU (a pair per workgroup), more (duos)
    cs.append(_case("claim_lin", "batch", LIN, {}, 400, 450, pairs=8))
    cs.append(_case("claim_aff", "batch", AFF, {}, 400, 450, pairs=8))
    cs.append(_case("pwg3_lin", "batch", LIN, {}, 400, 450, pairs=300))
    cs.append(_case("pwg3_aff_forced", "batch", AFF, {"mode": 5, "f2pwg": 1}, 400, 450, pairs=8))
    cs.append(_case("pwg3_aff_int32", "batch", (100, -3, 5, 2), {}, 660, 720, pairs=600))
    cs.append(_case("flow2_pwg", "batch", LIN, {"f3pwg": 0}, 400, 450, pairs=300))
    cs.append(_case("duo_auto", "batch", LIN, {}, 400, 450, pairs=600))
    duo = {"mode": 3, "W": 4, "C": 64}
    cs.append(_case("duo_lds_tab", "batch", LIN, duo, 400, 450, pairs=300))
    cs.append(_case("duo_lds_aff", "batch", AFF, {**duo, "duo_tab": 0}, 400, 450, pairs=300))
    cs.append(_case("duo_hbm_u16", "batch", LIN, {**duo, "duo_lds": 0, "duo16": 0}, 400, 450, pairs=300))
    cs.append(_case("duo_raw", "batch", LIN, {}, 400, 450, pairs=16, alphabet="protein"))
    cs.append(_case("bytes_pairwg", "batch", LIN, {"duo_raw": 0}, 400, 450, pairs=16, alphabet="protein"))
    return cs


_LOWER = np.arange(256, dtype=np.uint8)
_LOWER[np.frombuffer(b"ACGT", np.uint8)] = np.frombuffer(b"acgt", np.uint8)
_AA = np.frombuffer(b"ACDEFGHIKLMNPQRS", np.uint8)
_CODE = np.zeros(256, dtype=np.int64)
_CODE[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)


def _one_pair(engine, seed, n, m, alphabet):
    """A pair from the library's generator alone: b repeats a with about 6 % of its positions changed
    (long diagonals through every strip edge)."""
    ga, gb = engine.gen_pair(seed, 2 * max(n, m))
    if alphabet == "protein":   # sixteen letters from two bases each
        ga, gb = _AA[_CODE[ga[0::2]] * 4 + _CODE[ga[1::2]]], _AA[_CODE[gb[0::2]] * 4 + _CODE[gb[1::2]]]
    a = np.ascontiguousarray(ga[:n])
    b = np.resize(a, m).copy()
    mut = (_CODE[gb[:m]] == 0) & (np.arange(m) % 4 == 0) if alphabet != "protein" else np.arange(m) % 16 == 0
    b[mut] = gb[:m][mut]
    if alphabet == "lower":
        a, b = _LOWER[a], _LOWER[b]
    return a, np.ascontiguousarray(b)


def inputs(engine, idx, case):
    return [_one_pair(engine, 1000 * (idx + 1) + k, case["n"] + (k % 50 if case["kind"] == "batch" else 0),
                      case["m"], case["alphabet"]) for k in range(case["pairs"])]


def run_case(engine, idx, case, pairs=None):
    """Options and constants of `case` set from the defaults, its one call made: (stats fields, scores)."""
    import torch
    for k, v in DEFAULTS.items():
        engine.set_option(k, v)
    for k, v in case["options"].items():
        engine.set_option(k, v)
    engine.set_option("timeout", 5)
    prm = engine.Params(*case["params"])
    engine.set_params(prm)
    pairs = pairs if pairs is not None else inputs(engine, idx, case)
    a, b = pairs[0]
    if case["kind"] == "pair":
        scores = [engine.score(a, b, prm)]
    elif case["kind"] == "batch":
        scores = engine.score_batch(pairs, prm)
    else:
        arena = torch.from_numpy(np.concatenate([a, b])).cuda()
        out = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        if case["kind"] == "slab":
            engine.score_slab_device(arena.data_ptr(), 0, len(a), len(a), len(b), 0, 0, 0, out.data_ptr(),
                                     engine.SW_FLAG_DNA)
        else:
            engine.score_batch_device(arena.data_ptr(), [0], [len(a)], [len(a)], [len(b)], out.data_ptr())
        scores = [int(out.item())]
    st = engine.last_stats()
    return {k: int(st[k]) for k in FIELDS}, [int(s) for s in scores]


def reset(engine):
    for k, v in DEFAULTS.items():
        engine.set_option(k, v)
    engine.set_params(engine.Params())


def flow3_kernel(variant, C):
    """The flow3 kernel a launch ran, from its (variant, C); None for the other kernels."""
    bit = lambda i: bool(variant >> i & 1)   # noqa: E731
    if not (bit(6) or bit(10)):
        return None
    aff = "a" if bit(10) else ""
    if bit(15):
        return "sw_flow3r%s3p_kernel" % aff
    if bit(2):
        if bit(14):
            return "sw_flow3r45_kernel"
        if bit(13):
            return "sw_flow3r%s3%s_kernel" % (aff, "h" if bit(16) else "s" if bit(11) else "")
        if bit(11) or aff:
            return "sw_flow3r%s%s_kernel" % (aff, "s" if bit(11) else "")
        return "sw_flow3r_kernel<%d,%d>" % (C, bit(9))
    if bit(12):
        return "sw_flow3p_kernel<%d>" % bit(10)
    return "sw_flow3%s%s_kernel<%d,%d>" % (aff, "h" if bit(16) else "", C, bit(9))


FLOW3_KERNELS = frozenset(
    ["sw_flow3%s_kernel<%s>" % (f, t) for f in ("", "a", "h", "ah") for t in ("16,0", "32,0", "32,1")] +
    ["sw_flow3p_kernel<0>", "sw_flow3p_kernel<1>", "sw_flow3r_kernel<32,0>", "sw_flow3r_kernel<64,0>",
     "sw_flow3r_kernel<64,1>"] +
    ["sw_flow3%s_kernel" % k for k in ("ra", "rs", "ras", "r3", "ra3", "r3s", "ra3s", "r3h", "ra3h", "r45", "r3p",
                                       "ra3p")])


def coverage_missing(records):
    """What the records fail to reach of: every mode 0..5, each variant bit 0..17 set and clear, each of
    the 29 flow3 kernels, a cut pair and the four flow2 fallbacks."""
    missing = []
    stats = [r["stats"] for r in records]
    for mode in range(6):
        if not any(s["mode"] == mode for s in stats):
            missing.append("mode %d" % mode)
    for b in range(18):
        if not any(s["variant"] >> b & 1 for s in stats):
            missing.append("bit %d set" % b)
        if all(s["variant"] >> b & 1 for s in stats):
            missing.append("bit %d clear" % b)
    seen = {flow3_kernel(s["variant"], s["C"]) for s in stats}
    missing += sorted(FLOW3_KERNELS - seen)
    for opt in ("f3", "f3a", "f3slab", "f3pwg"):
        if not any(r["case"]["options"].get(opt) == 0 and r["stats"]["mode"] == 5 and
                   flow3_kernel(r["stats"]["variant"], r["stats"]["C"]) is None for r in records):
            missing.append("flow2 fallback with %s = 0" % opt)
    return missing


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch
    import concurrentproject_amd as engine
    import oracle
    records, bad = [], []
    try:
        for idx, case in enumerate(cases()):
            pairs = inputs(engine, idx, case)
            stats, scores = run_case(engine, idx, case, pairs)
            exp = oracle.score_batch(pairs, oracle.Params(*case["params"]))
            print(case["name"], stats, flow3_kernel(stats["variant"], stats["C"]), scores[:4], flush=True)
            if scores != exp:
                bad.append("%s: scores differ from the oracle" % case["name"])
            records.append({"case": case, "stats": stats, "scores": scores})
    finally:
        reset(engine)
    bad += coverage_missing(records)
    assert len(FLOW3_KERNELS) == 29 and len(records) <= 60
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(out, "w") as f:   # one record per line
        f.write('{"cus": %d, "records": [\n%s\n]}\n' % (cus, ",\n".join(json.dumps(r) for r in records)))
    if bad:
        sys.exit("not recorded cleanly:\n  " + "\n  ".join(bad))
    print("recorded %d cases on %d CUs -> %s" % (len(records), cus, out))


if __name__ == "__main__":
    main()
