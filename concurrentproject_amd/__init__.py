"""concurrentproject_amd -- MI355X (gfx950) Smith-Waterman score engine.

Python mirror of the reference's score interface (algoGPU.h:1-14 and the
harness calls of TestFileWithGPU.cpp:81-94) over the C-ABI of
``libswmi355.so`` (include/algoGPU.h).  Every call goes to the HIP kernels; there
is no CPU fallback: if the library is missing, importing the engine raises.

    import concurrentproject_amd as sw
    sw.SmithWatermanScoreCUDA(b"GATTACA", b"GCATGCU")      # -> 2
    sw.score_batch([(a0, b0), (a1, b1)])                     # -> [s0, s1]
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Iterable, Sequence

import numpy as np

__all__ = [
    "Params", "lib", "build", "SequentialSmithWatermanScoreGPU", "SmithWatermanLazyGPU",
    "SmithWatermanScoreCUDA", "SmithDiagonalGPU", "score", "score_batch", "score_batch_device",
    "set_params", "get_params", "set_option", "get_option", "last_stats", "gen_pair", "gen_batch",
    "SwError", "LIB_PATH", "SW_FLAG_DNA", "SW_FLAG_BYTES", "slab_bounds", "SlabBuffer", "slab_alloc",
    "ipc_open", "ipc_close", "score_slab_device", "Database", "Matrix", "score_matrix", "score_matrix_batch",
    "SW_MATRIX_FOLD_CASE", "Alignment", "align_matrix", "align_matrix_batch", "last_align_ms",
    "align_matrix_long", "align_long_plan", "last_align_long_ms", "coop_plan", "align_long_coop_plan",
    "Profile", "score_profile", "score_profile_batch", "align_profile", "align_profile_batch",
    "STANDARD_CODE", "FRAMES", "translate", "translated_range", "TranslatedAlignment", "score_matrix_translated",
    "score_matrix_translated_batch", "align_matrix_translated", "align_matrix_translated_batch",
]

HERE = os.path.dirname(os.path.abspath(__file__))
# SWMI355_LIB selects an instrumented build (tools/trace_flow.py); default: the in-tree library
LIB_PATH = os.environ.get("SWMI355_LIB") or os.path.join(HERE, "libswmi355.so")
SW_FLAG_DNA, SW_FLAG_BYTES = 1, 2


class SwError(RuntimeError):
    """A failed engine call (the C-ABI returned -1); the message is sw_last_error()."""


@dataclass(frozen=True)
class Params:
    """Scoring constants (main.cpp:20-23 defaults)."""
    match: int = 1
    mismatch: int = -1
    gap_init: int = 1
    gap_ext: int = 1


class _Stats(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_float), ("total_ms", ctypes.c_float), ("cells", ctypes.c_longlong),
                ("W", ctypes.c_int), ("C", ctypes.c_int), ("dna", ctypes.c_int), ("blocks", ctypes.c_int),
                ("waves_per_cu", ctypes.c_int), ("items", ctypes.c_int), ("boundary_bytes", ctypes.c_longlong),
                ("mode", ctypes.c_int), ("variant", ctypes.c_int)]


class _Alignment(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int), ("beg1", ctypes.c_int), ("end1", ctypes.c_int), ("beg2", ctypes.c_int),
                ("end2", ctypes.c_int), ("ncigar", ctypes.c_int), ("cigar_off", ctypes.c_longlong)]


class _AlignPlan(ctypes.Structure):
    _fields_ = [("strips", ctypes.c_int), ("ckpt_bytes", ctypes.c_longlong), ("strip_trace_bytes", ctypes.c_longlong),
                ("full_trace_bytes", ctypes.c_longlong)]


class _BandPlan(ctypes.Structure):
    _fields_ = [("dlo", ctypes.c_longlong), ("dhi", ctypes.c_longlong), ("cells", ctypes.c_longlong),
                ("trace_bytes", ctypes.c_longlong), ("full_trace_bytes", ctypes.c_longlong)]


class _CoopPlan(ctypes.Structure):
    _fields_ = [("W", ctypes.c_int), ("strips", ctypes.c_int), ("swap", ctypes.c_int), ("edge_bytes", ctypes.c_longlong),
                ("items", ctypes.c_longlong)]


class _AlignCoopPlan(ctypes.Structure):
    _fields_ = [("strips", ctypes.c_int), ("ckpt_bytes", ctypes.c_longlong), ("progress_bytes", ctypes.c_longlong),
                ("end_bytes", ctypes.c_longlong), ("window", ctypes.c_int), ("window_trace_bytes", ctypes.c_longlong)]


_lib = None


def build(verbose: bool = False) -> str:
    """Compile libswmi355.so in-tree for gfx950 (hipcc; no GPU needed)."""
    import subprocess
    cmd = ["make", "-j4", "-C", os.path.join(HERE, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.run(cmd, check=True)
    return LIB_PATH


def source_stamp() -> str:
    """sha256 over the engine's sources and build flags (csrc/*.hip, *.h, *.cpp, Makefile and
    include/algoGPU.h): identifies the kernels a profile was taken with, across rebuilds."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(HERE, "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) +
                   glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "*.inc")) +
                   [os.path.join(csrc, "Makefile"), os.path.join(HERE, "..", "include", "algoGPU.h")])
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def lib() -> ctypes.CDLL:
    """The loaded engine.  Raises if libswmi355.so has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libswmi355.so not built: run concurrentproject_amd.build() "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    u8p = ctypes.POINTER(ctypes.c_ubyte)
    i = ctypes.c_int
    for name in ("SequentialSmithWatermanScoreGPU", "SmithWatermanLazyGPU", "SmithWatermanScoreCUDA",
                 "SmithDiagonalGPU"):
        f = getattr(L, name)
        f.argtypes = [u8p, u8p, i, i]
        f.restype = i
    L.sw_set_params.argtypes = [i, i, i, i]
    L.sw_set_params.restype = i
    L.sw_get_params.argtypes = [ctypes.POINTER(i)] * 4
    L.sw_score_params.argtypes = [u8p, u8p, i, i, i, i, i, i]
    L.sw_score_params.restype = i
    L.sw_score_batch.argtypes = [ctypes.POINTER(u8p), ctypes.POINTER(i), ctypes.POINTER(u8p),
                                 ctypes.POINTER(i), i, ctypes.POINTER(i)]
    L.sw_score_batch.restype = i
    L.sw_score_batch_multi.argtypes = [ctypes.POINTER(u8p), ctypes.POINTER(i), ctypes.POINTER(u8p),
                                       ctypes.POINTER(i), i, ctypes.POINTER(i), i]
    L.sw_score_batch_multi.restype = i
    L.sw_batch_shard.argtypes = [i, i, i, ctypes.POINTER(i), ctypes.POINTER(i)]
    L.sw_batch_shard.restype = i
    if hasattr(L, "sw_batch_gather_plan"):   # (absent from pre-r05 builds that tools/ab.sh --libs may load)
        L.sw_batch_gather_plan.argtypes = [i, i, ctypes.POINTER(i), ctypes.POINTER(i)]
        L.sw_batch_gather_plan.restype = i
    L.sw_score_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(i),
                                        ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(i), i, ctypes.c_void_p, i,
                                        ctypes.c_void_p]
    L.sw_score_batch_device.restype = i
    L.sw_stream_status.argtypes = [ctypes.c_void_p]
    L.sw_stream_status.restype = i
    L.sw_set_option.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
    L.sw_set_option.restype = i
    L.sw_get_option.argtypes = [ctypes.c_char_p]
    L.sw_get_option.restype = ctypes.c_longlong
    L.sw_last_stats.argtypes = [ctypes.POINTER(_Stats)]
    L.sw_last_stats.restype = i
    L.sw_last_error.restype = ctypes.c_char_p
    L.sw_version.restype = i
    L.sw_gen_pair.argtypes = [ctypes.c_uint64, i, u8p, u8p]
    L.sw_gen_batch.argtypes = [ctypes.c_uint64, i, i, u8p]
    vp = ctypes.c_void_p
    L.sw_slab_bounds.argtypes = [ctypes.c_longlong, i, i, i, ctypes.POINTER(ctypes.c_longlong)]
    L.sw_slab_bounds.restype = i
    if hasattr(L, "sw_split_bounds"):   # (absent from older builds that SWMI355_LIB may name for an A/B)
        L.sw_split_bounds.argtypes = [i, ctypes.POINTER(i), ctypes.POINTER(i)]
        L.sw_split_bounds.restype = i
    L.sw_score_slab_device.argtypes = [vp, ctypes.c_int64, i, ctypes.c_int64, i, vp, vp, ctypes.c_uint, vp, i, vp]
    L.sw_score_slab_device.restype = i
    L.sw_slab_alloc.argtypes = [i, ctypes.POINTER(vp), ctypes.c_char_p]
    L.sw_slab_alloc.restype = i
    L.sw_slab_free.argtypes = [vp]
    L.sw_slab_free.restype = i
    L.sw_ipc_open.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
    L.sw_ipc_open.restype = i
    L.sw_ipc_close.argtypes = [vp]
    L.sw_ipc_close.restype = i
    # FASTA databases (include/algoGPU.h)
    L.sw_db_open.argtypes = [ctypes.c_char_p]
    L.sw_db_open.restype = vp
    L.sw_db_from_fasta.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
    L.sw_db_from_fasta.restype = vp
    L.sw_db_save.argtypes = [vp, ctypes.c_char_p]
    L.sw_db_save.restype = i
    L.sw_db_count.argtypes = [vp]
    L.sw_db_count.restype = i
    L.sw_db_residues.argtypes = [vp]
    L.sw_db_residues.restype = ctypes.c_longlong
    L.sw_db_record.argtypes = [vp, i, ctypes.POINTER(u8p), ctypes.POINTER(i), ctypes.POINTER(ctypes.c_char_p)]
    L.sw_db_record.restype = i
    L.sw_db_search.argtypes = [vp, u8p, i, ctypes.POINTER(i)]
    L.sw_db_search.restype = i
    L.sw_db_search_db.argtypes = [vp, vp, ctypes.POINTER(i)]
    L.sw_db_search_db.restype = i
    L.sw_db_close.argtypes = [vp]
    L.sw_db_close.restype = None
    # substitution matrices (include/algoGPU.h)
    i8p = ctypes.POINTER(ctypes.c_byte)
    L.sw_matrix_create.argtypes = [u8p, i, i8p, i, i]
    L.sw_matrix_create.restype = vp
    L.sw_matrix_parse.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
    L.sw_matrix_parse.restype = vp
    L.sw_matrix_open.argtypes = [ctypes.c_char_p]
    L.sw_matrix_open.restype = vp
    L.sw_matrix_size.argtypes = [vp]
    L.sw_matrix_size.restype = i
    L.sw_matrix_symbols.argtypes = [vp, u8p]
    L.sw_matrix_symbols.restype = i
    L.sw_matrix_score.argtypes = [vp, ctypes.c_ubyte, ctypes.c_ubyte, ctypes.POINTER(i)]
    L.sw_matrix_score.restype = i
    L.sw_matrix_free.argtypes = [vp]
    L.sw_matrix_free.restype = None
    L.sw_score_matrix.argtypes = [vp, u8p, u8p, i, i, i, i]
    L.sw_score_matrix.restype = i
    L.sw_score_matrix_batch.argtypes = [vp, ctypes.POINTER(u8p), ctypes.POINTER(i), ctypes.POINTER(u8p),
                                        ctypes.POINTER(i), i, i, i, ctypes.POINTER(i)]
    L.sw_score_matrix_batch.restype = i
    L.sw_db_search_matrix.argtypes = [vp, vp, u8p, i, i, i, ctypes.POINTER(i)]
    L.sw_db_search_matrix.restype = i
    L.sw_db_search_db_matrix.argtypes = [vp, vp, vp, i, i, ctypes.POINTER(i)]
    L.sw_db_search_db_matrix.restype = i
    # alignments (include/algoGPU.h sw_align_*; absent from older builds that SWMI355_LIB may name for an A/B)
    ll = ctypes.c_longlong
    if hasattr(L, "sw_align_matrix_batch"):
        for name in ("sw_align_matrix_batch", "sw_align_matrix_cpu"):
            f = getattr(L, name)
            f.argtypes = [vp, ctypes.POINTER(u8p), ctypes.POINTER(i), ctypes.POINTER(u8p), ctypes.POINTER(i), i, i, i,
                          ctypes.POINTER(_Alignment), ctypes.POINTER(ctypes.c_uint), ll, ctypes.POINTER(ll)]
            f.restype = i
        L.sw_db_align_matrix.argtypes = [vp, vp, u8p, i, ctypes.POINTER(i), i, i, i, ctypes.POINTER(_Alignment),
                                         ctypes.POINTER(ctypes.c_uint), ll, ctypes.POINTER(ll)]
        L.sw_db_align_matrix.restype = i
        L.sw_last_align_ms.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.sw_last_align_ms.restype = None
    if hasattr(L, "sw_align_matrix_long"):   # checkpointed traceback of long pairs
        L.sw_align_matrix_long.argtypes = L.sw_align_matrix_batch.argtypes
        L.sw_align_matrix_long.restype = i
        L.sw_db_align_matrix_long.argtypes = L.sw_db_align_matrix.argtypes
        L.sw_db_align_matrix_long.restype = i
        L.sw_align_long_plan.argtypes = [i, i, ctypes.POINTER(_AlignPlan)]
        L.sw_align_long_plan.restype = i
        fp = ctypes.POINTER(ctypes.c_float)
        L.sw_last_align_long_ms.argtypes = [fp, fp, fp, ctypes.POINTER(i)]
        L.sw_last_align_long_ms.restype = None
    if hasattr(L, "sw_align_matrix_batch_mode"):   # global and semi-global alignment (SW_MODE_*)
        L.sw_score_matrix_batch_mode.argtypes = [vp, ctypes.POINTER(u8p), ctypes.POINTER(i), ctypes.POINTER(u8p),
                                                 ctypes.POINTER(i), i, i, i, i, ctypes.POINTER(i)]
        L.sw_score_matrix_batch_mode.restype = i
        for name in ("sw_align_matrix_batch_mode", "sw_align_matrix_cpu_mode"):
            f = getattr(L, name)
            f.argtypes = [vp, ctypes.POINTER(u8p), ctypes.POINTER(i), ctypes.POINTER(u8p), ctypes.POINTER(i), i, i, i, i,
                          ctypes.POINTER(_Alignment), ctypes.POINTER(ctypes.c_uint), ll, ctypes.POINTER(ll)]
            f.restype = i
        L.sw_db_search_matrix_mode.argtypes = [vp, vp, u8p, i, i, i, i, ctypes.POINTER(i)]
        L.sw_db_search_matrix_mode.restype = i
        L.sw_db_align_matrix_mode.argtypes = [vp, vp, u8p, i, ctypes.POINTER(i), i, i, i, i, ctypes.POINTER(_Alignment),
                                              ctypes.POINTER(ctypes.c_uint), ll, ctypes.POINTER(ll)]
        L.sw_db_align_matrix_mode.restype = i
    if hasattr(L, "sw_align_matrix_batch_band"):   # banded alignment (include/algoGPU.h sw_*_band)
        L.sw_score_matrix_batch_band.argtypes = [vp, ctypes.POINTER(u8p), ctypes.POINTER(i), ctypes.POINTER(u8p),
                                                 ctypes.POINTER(i), i, i, i, i, i, ctypes.POINTER(i)]
        L.sw_score_matrix_batch_band.restype = i
        for name in ("sw_align_matrix_batch_band", "sw_align_matrix_cpu_band"):
            f = getattr(L, name)
            f.argtypes = [vp, ctypes.POINTER(u8p), ctypes.POINTER(i), ctypes.POINTER(u8p), ctypes.POINTER(i), i, i, i, i, i,
                          ctypes.POINTER(_Alignment), ctypes.POINTER(ctypes.c_uint), ll, ctypes.POINTER(ll)]
            f.restype = i
        L.sw_band_plan.argtypes = [i, i, i, ctypes.POINTER(_BandPlan)]
        L.sw_band_plan.restype = i
    if hasattr(L, "sw_score_matrix_batch_coop"):   # one pair's strips on many waves (include/algoGPU.h)
        L.sw_score_matrix_batch_coop.argtypes = [vp, ctypes.POINTER(u8p), ctypes.POINTER(i), ctypes.POINTER(u8p),
                                                 ctypes.POINTER(i), i, i, i, i, ctypes.POINTER(i)]
        L.sw_score_matrix_batch_coop.restype = i
        L.sw_matrix_coop_plan.argtypes = [i, i, i, ctypes.POINTER(_CoopPlan)]
        L.sw_matrix_coop_plan.restype = i
    if hasattr(L, "sw_align_matrix_long_coop"):   # long pairs on many waves (include/algoGPU.h)
        L.sw_align_matrix_long_coop.argtypes = L.sw_align_matrix_batch.argtypes
        L.sw_align_matrix_long_coop.restype = i
        L.sw_db_align_matrix_long_coop.argtypes = L.sw_db_align_matrix.argtypes
        L.sw_db_align_matrix_long_coop.restype = i
        L.sw_align_long_coop_plan.argtypes = [i, i, ctypes.POINTER(_AlignCoopPlan)]
        L.sw_align_long_coop_plan.restype = i
    if hasattr(L, "sw_align_matrix_long_mode"):   # the long path, global and semi-global (include/algoGPU.h)
        for name in ("sw_align_matrix_long_mode", "sw_align_matrix_long_coop_mode"):
            f = getattr(L, name)
            f.argtypes = L.sw_align_matrix_batch_mode.argtypes
            f.restype = i
        for name in ("sw_db_align_matrix_long_mode", "sw_db_align_matrix_long_coop_mode"):
            f = getattr(L, name)
            f.argtypes = L.sw_db_align_matrix_mode.argtypes
            f.restype = i
    if hasattr(L, "sw_profile_create"):   # position-specific scoring (include/algoGPU.h sw_profile_*)
        L.sw_profile_create.argtypes = [u8p, i, i8p, i, i, i]
        L.sw_profile_create.restype = vp
        L.sw_profile_from_matrix.argtypes = [vp, u8p, i]
        L.sw_profile_from_matrix.restype = vp
        L.sw_profile_parse.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
        L.sw_profile_parse.restype = vp
        L.sw_profile_open.argtypes = [ctypes.c_char_p]
        L.sw_profile_open.restype = vp
        for name in ("sw_profile_length", "sw_profile_size"):
            f = getattr(L, name)
            f.argtypes = [vp]
            f.restype = i
        L.sw_profile_symbols.argtypes = [vp, u8p]
        L.sw_profile_symbols.restype = i
        L.sw_profile_score.argtypes = [vp, i, ctypes.c_ubyte, ctypes.POINTER(i)]
        L.sw_profile_score.restype = i
        L.sw_profile_free.argtypes = [vp]
        L.sw_profile_free.restype = None
        L.sw_score_profile_batch.argtypes = [vp, ctypes.POINTER(u8p), ctypes.POINTER(i), i, i, i, i, ctypes.POINTER(i)]
        L.sw_score_profile_batch.restype = i
        for name in ("sw_align_profile_batch", "sw_align_profile_cpu"):
            f = getattr(L, name)
            f.argtypes = [vp, ctypes.POINTER(u8p), ctypes.POINTER(i), i, i, i, i, ctypes.POINTER(_Alignment),
                          ctypes.POINTER(ctypes.c_uint), ll, ctypes.POINTER(ll)]
            f.restype = i
        L.sw_db_search_profile.argtypes = [vp, vp, i, i, i, ctypes.POINTER(i)]
        L.sw_db_search_profile.restype = i
        L.sw_db_align_profile.argtypes = [vp, vp, ctypes.POINTER(i), i, i, i, i, ctypes.POINTER(_Alignment),
                                          ctypes.POINTER(ctypes.c_uint), ll, ctypes.POINTER(ll)]
        L.sw_db_align_profile.restype = i
    if hasattr(L, "sw_translate"):   # translated search (include/algoGPU.h sw_*_translated*)
        ip = ctypes.POINTER(i)
        L.sw_standard_code.argtypes = [u8p]
        L.sw_standard_code.restype = None
        L.sw_translate.argtypes = [u8p, i, i, u8p, u8p, i]
        L.sw_translate.restype = i
        L.sw_translated_range.argtypes = [i, i, i, i, ip, ip]
        L.sw_translated_range.restype = i
        L.sw_translated_tables.argtypes = [vp, u8p, u8p, u8p]
        L.sw_translated_tables.restype = i
        L.sw_score_matrix_translated_batch.argtypes = [vp, ctypes.POINTER(u8p), ip, ctypes.POINTER(u8p), ip, i, i, i, i, u8p, ip]
        L.sw_score_matrix_translated_batch.restype = i
        for name in ("sw_align_matrix_translated_batch", "sw_align_matrix_translated_cpu"):
            f = getattr(L, name)
            f.argtypes = [vp, ctypes.POINTER(u8p), ip, ctypes.POINTER(u8p), ip, ip, i, i, i, i, u8p,
                          ctypes.POINTER(_Alignment), ctypes.POINTER(ctypes.c_uint), ll, ctypes.POINTER(ll)]
            f.restype = i
        L.sw_db_search_matrix_translated.argtypes = [vp, vp, u8p, i, i, i, i, u8p, ip]
        L.sw_db_search_matrix_translated.restype = i
        L.sw_db_align_matrix_translated.argtypes = [vp, vp, u8p, i, ip, ip, i, i, i, i, u8p, ctypes.POINTER(_Alignment),
                                                    ctypes.POINTER(ctypes.c_uint), ll, ctypes.POINTER(ll)]
        L.sw_db_align_matrix_translated.restype = i
    _lib = L
    return L


def _u8(a) -> np.ndarray:
    if isinstance(a, str):
        a = a.encode("latin-1")
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


def _ptr(arr: np.ndarray):
    return arr.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))


def _check(rc: int) -> int:
    if rc < 0:
        raise SwError(lib().sw_last_error().decode(errors="replace"))
    return rc


def _pair_call(fname: str, seq1, seq2) -> int:
    a, b = _u8(seq1), _u8(seq2)
    return _check(getattr(lib(), fname)(_ptr(a), _ptr(b), len(a), len(b)))


# ---- the reference's algoGPU.h surface ----------------------------------------------------

def SequentialSmithWatermanScoreGPU(seq1, seq2) -> int:
    """algoGPU.h:5 (simpleGPU.cu:109): score of (seq1, seq2)."""
    return _pair_call("SequentialSmithWatermanScoreGPU", seq1, seq2)


def SmithWatermanLazyGPU(seq1, seq2) -> int:
    """algoGPU.h:7 (cudaLazy.cu:58)."""
    return _pair_call("SmithWatermanLazyGPU", seq1, seq2)


def SmithWatermanScoreCUDA(seq1, seq2) -> int:
    """algoGPU.h:9 (cudaSmithM.cu:128)."""
    return _pair_call("SmithWatermanScoreCUDA", seq1, seq2)


def SmithDiagonalGPU(seq1, seq2) -> int:
    """SmithDiagonalGPUrefactored.cu:174 (linear gap = G_INIT per residue)."""
    return _pair_call("SmithDiagonalGPU", seq1, seq2)


# ---- extensions ---------------------------------------------------------------------------

def score(seq1, seq2, params: Params | None = None) -> int:
    """Best local-alignment score; ``params`` overrides the process-wide constants for this call."""
    if params is None:
        return SmithWatermanScoreCUDA(seq1, seq2)
    a, b = _u8(seq1), _u8(seq2)
    return _check(lib().sw_score_params(_ptr(a), _ptr(b), len(a), len(b), params.match, params.mismatch,
                                        params.gap_init, params.gap_ext))


def score_batch(pairs: Iterable[Sequence], params: Params | None = None, ngpus: int = 0) -> list:
    """Scores of many independent pairs in one launch (sw_score_batch); with ngpus >= 1,
    sharded over the first ngpus GPUs with an RCCL gather of the scores
    (sw_score_batch_multi)."""
    arrs = [(_u8(a), _u8(b)) for a, b in pairs]
    n = len(arrs)
    if n == 0:
        return []
    u8p = ctypes.POINTER(ctypes.c_ubyte)
    A = (u8p * n)(*[_ptr(x) for x, _ in arrs])
    B = (u8p * n)(*[_ptr(y) for _, y in arrs])
    AL = (ctypes.c_int * n)(*[len(x) for x, _ in arrs])
    BL = (ctypes.c_int * n)(*[len(y) for _, y in arrs])
    out = (ctypes.c_int * n)()
    old = None
    if params is not None:
        old = get_params()
        set_params(params)
    try:
        if ngpus:
            _check(lib().sw_score_batch_multi(A, AL, B, BL, n, out, ngpus))
        else:
            _check(lib().sw_score_batch(A, AL, B, BL, n, out))
    finally:
        if old is not None:
            set_params(old)
    return list(out)


def batch_shard(npairs: int, ngpus: int, rank: int) -> tuple:
    """[lo, hi) of rank `rank`'s contiguous shard in sw_score_batch_multi (no GPU call)."""
    lo, hi = ctypes.c_int(), ctypes.c_int()
    _check(lib().sw_batch_shard(npairs, ngpus, rank, ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def batch_gather_plan(npairs: int, ngpus: int) -> list:
    """[(count, offset)] per device of sw_score_batch_multi's RCCL gather to device 0 (no GPU call)."""
    cnt, off = (ctypes.c_int * max(ngpus, 1))(), (ctypes.c_int * max(ngpus, 1))()
    _check(lib().sw_batch_gather_plan(npairs, ngpus, cnt, off))
    return [(cnt[r], off[r]) for r in range(ngpus)]


def score_batch_device(d_arena_ptr: int, a_off, alen, b_off, blen, d_scores_ptr: int, flags: int = 0,
                       stream: int | None = None) -> None:
    """Sequences already in device memory (arena pointer + byte offsets).  Asynchronous on ``stream``."""
    npairs = len(alen)
    ao = (ctypes.c_int64 * npairs)(*[int(x) for x in a_off])
    bo = (ctypes.c_int64 * npairs)(*[int(x) for x in b_off])
    al = (ctypes.c_int * npairs)(*[int(x) for x in alen])
    bl = (ctypes.c_int * npairs)(*[int(x) for x in blen])
    _check(lib().sw_score_batch_device(ctypes.c_void_p(d_arena_ptr), ao, al, bo, bl, npairs,
                                       ctypes.c_void_p(d_scores_ptr), flags,
                                       ctypes.c_void_p(stream) if stream else None))


def stream_status(stream: int | None = None) -> None:
    _check(lib().sw_stream_status(ctypes.c_void_p(stream) if stream else None))


# ---- one pair in column slabs across GPUs (dist.ColumnSlabs drives these) -----------------

SW_IPC_HANDLE_BYTES = 64


def slab_bounds(n: int, m: int, nslabs: int, flags: int) -> list:
    """Column bounds [b_0 = 0, ..., b_nslabs = n] of nslabs slabs; every slab but the
    last is a multiple of the planned kernel's column quantum (63 or 64*W)."""
    out = (ctypes.c_longlong * (nslabs + 1))()
    _check(lib().sw_slab_bounds(int(n), int(m), int(nslabs), int(flags), out))
    return [int(x) for x in out]


def split_bounds(n: int):
    """Where option f3split cuts one pair of n columns: (cut, lead, strips of both halves), or
    None when n is too narrow (each half needs two strips of 126 new columns)."""
    c, lead = ctypes.c_int(), ctypes.c_int()
    strips = _check(lib().sw_split_bounds(int(n), ctypes.byref(c), ctypes.byref(lead)))
    return (c.value, lead.value, strips) if strips else None


class SlabBuffer:
    """A slab's inflow edge: m zeroed 16-byte granules in device memory, and the
    IPC handle under which the rank that writes it maps it."""

    def __init__(self, m: int):
        p = ctypes.c_void_p()
        h = ctypes.create_string_buffer(SW_IPC_HANDLE_BYTES)
        kind = _check(lib().sw_slab_alloc(int(m), ctypes.byref(p), h))
        self.ptr = int(p.value)
        self.handle = h.raw
        self.fine_grained = kind == 1
        self.m = m

    def free(self) -> None:
        if self.ptr:
            _check(lib().sw_slab_free(ctypes.c_void_p(self.ptr)))
            self.ptr = 0


def slab_alloc(m: int) -> SlabBuffer:
    return SlabBuffer(m)


def ipc_open(handle: bytes) -> int:
    """Map another process's slab buffer (hipIpcOpenMemHandle); returns its device address here."""
    p = ctypes.c_void_p()
    _check(lib().sw_ipc_open(handle, ctypes.byref(p)))
    return int(p.value)


def ipc_close(ptr: int) -> None:
    if ptr:
        _check(lib().sw_ipc_close(ctypes.c_void_p(ptr)))


def score_slab_device(d_arena_ptr: int, col_off: int, n: int, row_off: int, m: int, d_inflow: int,
                      d_outflow: int, epoch: int, d_score_ptr: int, flags: int, stream: int | None = None) -> None:
    """One column slab (sw_score_slab_device): *d_score = max H over its cells."""
    _check(lib().sw_score_slab_device(ctypes.c_void_p(d_arena_ptr), int(col_off), int(n), int(row_off), int(m),
                                      ctypes.c_void_p(d_inflow) if d_inflow else None,
                                      ctypes.c_void_p(d_outflow) if d_outflow else None, int(epoch),
                                      ctypes.c_void_p(d_score_ptr), int(flags),
                                      ctypes.c_void_p(stream) if stream else None))


def set_params(p: Params) -> None:
    _check(lib().sw_set_params(p.match, p.mismatch, p.gap_init, p.gap_ext))


def get_params() -> Params:
    v = [ctypes.c_int() for _ in range(4)]
    lib().sw_get_params(*[ctypes.byref(x) for x in v])
    return Params(*[x.value for x in v])


def set_option(key: str, value: int) -> None:
    if lib().sw_set_option(key.encode(), int(value)) != 0:
        raise SwError("bad option %s=%r" % (key, value))


def get_option(key: str) -> int:
    return int(lib().sw_get_option(key.encode()))


def last_stats() -> dict:
    s = _Stats()
    lib().sw_last_stats(ctypes.byref(s))
    return {k: getattr(s, k) for k, _ in _Stats._fields_}


def gen_pair(seed: int, length: int) -> tuple:
    """cudaSmithM.cu:200-212 synthetic pair: mt19937_64(seed), a[i] then b[i] over 'ACGT'."""
    a = np.empty(length, dtype=np.uint8)
    b = np.empty(length, dtype=np.uint8)
    lib().sw_gen_pair(seed, length, _ptr(a), _ptr(b))
    return a, b


def gen_batch(seed_base: int, npairs: int, length: int) -> np.ndarray:
    """npairs pairs (pair k seeded seed_base+k) as one arena [a_0|b_0|a_1|b_1|...]."""
    arena = np.empty(2 * length * npairs, dtype=np.uint8)
    lib().sw_gen_batch(seed_base, npairs, length, _ptr(arena))
    return arena


# ---- substitution-matrix scoring (include/algoGPU.h sw_matrix_*) ---------------------------

SW_MATRIX_FOLD_CASE = 1


class Matrix:
    """A substitution matrix: K distinct byte symbols and a K x K table, ``scores[i][j]`` scoring
    symbol i of seq1 / the query against symbol j of seq2 / the record (it need not be symmetric).
    ``other``: the index every byte outside the alphabet maps to, or -1 (such a byte is then an
    error); ``fold_case``: a-z score as A-Z wherever the lower-case byte is not itself a symbol.
    No named matrix is built in: ``Matrix.open("BLOSUM62")`` reads a file in the NCBI text format.
    Immutable; usable from any thread."""

    def __init__(self, symbols=None, scores=None, other: int = -1, fold_case: bool = False, _handle=None):
        if _handle is None:
            sym = _u8(symbols)
            tab = np.ascontiguousarray(scores, dtype=np.int64).reshape(-1)
            if tab.size != len(sym) * len(sym):
                raise SwError("matrix: the table is not %d x %d" % (len(sym), len(sym)))
            if tab.size and (tab.min() < -127 or tab.max() > 127):
                raise SwError("matrix: an entry is outside [-127, 127]")
            t8 = tab.astype(np.int8)
            _handle = lib().sw_matrix_create(_ptr(sym), len(sym), t8.ctypes.data_as(ctypes.POINTER(ctypes.c_byte)),
                                             int(other), SW_MATRIX_FOLD_CASE if fold_case else 0)
        if not _handle:
            raise SwError(lib().sw_last_error().decode(errors="replace"))
        self._h = ctypes.c_void_p(_handle)

    @classmethod
    def parse(cls, text) -> "Matrix":
        """From the NCBI text format ('#' comments, a header line of symbols, K labelled rows)."""
        if isinstance(text, str):
            text = text.encode("latin-1")
        return cls(_handle=lib().sw_matrix_parse(text, len(text)) or 0)

    @classmethod
    def open(cls, path) -> "Matrix":
        return cls(_handle=lib().sw_matrix_open(os.fsencode(path)) or 0)

    @classmethod
    def equality(cls, symbols, match: int, mismatch: int) -> "Matrix":
        """The table of a byte-equality scoring over the distinct bytes ``symbols`` (at most 32):
        ``match`` on the diagonal, ``mismatch`` elsewhere.  With it, alignments under the
        reference's own scoring (``Params``) need no matrix file.  It is also the way to global and
        semi-global alignment (``mode=``) under equality scoring: those modes take a matrix."""
        sym = bytes(sorted(set(_u8(symbols).tolist())))
        if not 1 <= len(sym) <= 32:
            raise SwError("equality matrix: %d distinct bytes (need 1 to 32)" % len(sym))
        k = len(sym)
        return cls(sym, np.where(np.eye(k, dtype=bool), int(match), int(mismatch)))

    def _handle(self):
        if self._h is None:
            raise SwError("matrix is closed")
        return self._h

    @property
    def symbols(self) -> bytes:
        k = lib().sw_matrix_size(self._handle())
        out = np.zeros(max(k, 1), dtype=np.uint8)
        _check(lib().sw_matrix_symbols(self._handle(), _ptr(out)))
        return out[:k].tobytes()

    def score(self, a, b) -> int:
        """The entry for bytes (a, b), through the byte-to-code map the kernel uses."""
        out = ctypes.c_int()
        _check(lib().sw_matrix_score(self._handle(), int(_u8(a)[0]), int(_u8(b)[0]), ctypes.byref(out)))
        return out.value

    def close(self) -> None:
        if self._h is not None and self._h.value:
            lib().sw_matrix_free(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SW_MODE_LOCAL, SW_MODE_GLOBAL, SW_MODE_SEMIGLOBAL = 0, 1, 2
_MODES = {"local": SW_MODE_LOCAL, "global": SW_MODE_GLOBAL, "semiglobal": SW_MODE_SEMIGLOBAL}


def _mode(mode) -> int:
    """The SW_MODE_* value of ``mode``: "local", "global" (seq1 and seq2 end to end) or "semiglobal"
    (seq1, the query, end to end inside seq2, the record, whose flanks are free)."""
    try:
        return _MODES[mode]
    except (KeyError, TypeError):
        raise ValueError("unknown alignment mode %r: use 'local', 'global' or 'semiglobal'" % (mode,)) from None


def _band(band) -> int:
    """``band`` as the library takes it: a C int (the library refuses a negative one by name)."""
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)):
        raise ValueError("band=%r: a band is a whole number >= 0, or None" % (band,))
    return max(-1, min(int(band), 2 ** 31 - 1))


def score_matrix(seq1, seq2, matrix: Matrix, gap_init: int, gap_ext: int, mode: str = "local",
                 band: int | None = None, coop: bool = False) -> int:
    """Best local-alignment score under ``matrix``; a gap of L residues costs gap_init + (L-1)*gap_ext
    (BLAST's "open 11, extend 1" is gap_init=12, gap_ext=1).  ``mode="global"`` / ``"semiglobal"``:
    the end-to-end / query-inside-record score (include/algoGPU.h SW_MODE_*), which may be negative.
    ``band`` and ``coop``: see :func:`score_matrix_batch`."""
    if _mode(mode) != SW_MODE_LOCAL or band is not None or coop:
        return score_matrix_batch([(seq1, seq2)], matrix, gap_init, gap_ext, mode=mode, band=band, coop=coop)[0]
    a, b = _u8(seq1), _u8(seq2)
    return _check(lib().sw_score_matrix(matrix._handle(), _ptr(a), _ptr(b), len(a), len(b), int(gap_init), int(gap_ext)))


def score_matrix_batch(pairs: Iterable[Sequence], matrix: Matrix, gap_init: int, gap_ext: int, mode: str = "local",
                       band: int | None = None, coop: bool = False) -> list:
    """Scores of many independent pairs under ``matrix`` in one launch (sw_score_matrix_batch; with
    ``mode`` "global" or "semiglobal" sw_score_matrix_batch_mode: one launch is one mode).
    ``band=B`` (sw_score_matrix_batch_band, any mode): only the cells (i, j) of a pair with
    min(0, m - n) - B <= j - i <= max(0, m - n) + B exist (include/algoGPU.h; :func:`band_plan`).
    ``coop=True`` (sw_score_matrix_batch_coop, any mode, no band): the same scores with the strips of
    every pair on as many waves as it has strips, for one or a few long pairs (:func:`coop_plan`)."""
    am = _mode(mode)
    if coop:
        if band is not None:
            raise ValueError("band= is not built for coop=True (the cooperative score path)")
        if not isinstance(matrix, Matrix):
            raise ValueError("coop=True needs a substitution matrix (Matrix.equality gives equality scoring as one)")
        return _score_matrix_batch(pairs, matrix, gap_init, gap_ext, am, coop=True)
    if band is not None:
        if not isinstance(matrix, Matrix):
            raise ValueError("band= needs a substitution matrix (Matrix.equality gives equality scoring as one)")
        return _score_matrix_batch(pairs, matrix, gap_init, gap_ext, am, _band(band))
    if am != SW_MODE_LOCAL and not isinstance(matrix, Matrix):
        raise ValueError("mode=%r needs a substitution matrix (Matrix.equality gives equality scoring as one)" % mode)
    return _score_matrix_batch(pairs, matrix, gap_init, gap_ext, am if am != SW_MODE_LOCAL else None)


def _score_matrix_batch(pairs, matrix, gap_init: int, gap_ext: int, am, band=None, coop=False) -> list:
    """am None: sw_score_matrix_batch; else sw_score_matrix_batch_mode with that SW_MODE_* value, or with
    a band sw_score_matrix_batch_band, or (coop) sw_score_matrix_batch_coop."""
    arrs = [(_u8(a), _u8(b)) for a, b in pairs]
    n = len(arrs)
    if n == 0:
        return []
    u8p = ctypes.POINTER(ctypes.c_ubyte)
    A = (u8p * n)(*[_ptr(x) for x, _ in arrs])
    B = (u8p * n)(*[_ptr(y) for _, y in arrs])
    AL = (ctypes.c_int * n)(*[len(x) for x, _ in arrs])
    BL = (ctypes.c_int * n)(*[len(y) for _, y in arrs])
    out = (ctypes.c_int * n)()
    if coop:
        _check(lib().sw_score_matrix_batch_coop(matrix._handle(), A, AL, B, BL, n, int(gap_init), int(gap_ext), am, out))
    elif band is not None:
        _check(lib().sw_score_matrix_batch_band(matrix._handle(), A, AL, B, BL, n, int(gap_init), int(gap_ext), am, band, out))
    elif am is not None:
        _check(lib().sw_score_matrix_batch_mode(matrix._handle(), A, AL, B, BL, n, int(gap_init), int(gap_ext), am, out))
    else:
        _check(lib().sw_score_matrix_batch(matrix._handle(), A, AL, B, BL, n, int(gap_init), int(gap_ext), out))
    return list(out)


# ---- alignments (include/algoGPU.h sw_align_*) ------------------------------------------------------

@dataclass(frozen=True)
class Alignment:
    """One alignment: its score, the half-open ranges [beg1, end1) of seq1 and [beg2, end2)
    of seq2 it covers, and its operations: ``ops`` is a tuple of (length, op) with op one of "M" (a
    residue of seq1 aligned with one of seq2), "I" (a residue of seq1 against a gap), "D" (a
    residue of seq2 against a gap); ``cigar`` the same as a string such as ``12M2D40M``.  Local: a
    pair with score 0 has empty ranges at 0 and no operations, and an alignment begins and ends
    with an M.  Global covers [0, n) x [0, m) and semi-global [0, n) x [beg2, end2); both may begin
    or end with a gap and have a negative score, and a score of 0 says nothing about emptiness."""
    score: int
    beg1: int
    end1: int
    beg2: int
    end2: int
    ops: tuple = ()

    @property
    def cigar(self) -> str:
        return "".join("%d%s" % (n, op) for n, op in self.ops)

    def columns(self, seq1, seq2):
        """The aligned columns as (row1, row2) byte strings with '-' for a gap."""
        a, b = _u8(seq1), _u8(seq2)
        i, j = self.beg1, self.beg2
        r1, r2 = [], []
        for n, op in self.ops:
            if op == "M":
                r1.append(a[i:i + n].tobytes())
                r2.append(b[j:j + n].tobytes())
                i, j = i + n, j + n
            elif op == "I":
                r1.append(a[i:i + n].tobytes())
                r2.append(b"-" * n)
                i += n
            else:
                r1.append(b"-" * n)
                r2.append(b[j:j + n].tobytes())
                j += n
        return b"".join(r1), b"".join(r2)

    def identities(self, seq1, seq2) -> int:
        """Aligned pairs (M columns) whose two bytes are equal."""
        r1, r2 = self.columns(seq1, seq2)
        return sum(1 for x, y in zip(r1, r2) if x == y and x != 0x2D)

    def pretty(self, seq1, seq2) -> str:
        """The usual three lines: seq1's row, '|' under equal bytes, seq2's row."""
        r1, r2 = self.columns(seq1, seq2)
        mid = "".join("|" if x == y and x != 0x2D else " " for x, y in zip(r1, r2))
        return "%s\n%s\n%s" % (r1.decode("latin-1"), mid, r2.decode("latin-1"))


_OPS = "MID"


def _alignments(out, cigar) -> list:
    res = []
    for o in out:
        ent = cigar[o.cigar_off:o.cigar_off + o.ncigar]
        res.append(Alignment(o.score, o.beg1, o.end1, o.beg2, o.end2, tuple((int(e) >> 4, _OPS[int(e) & 15]) for e in ent)))
    return res


def _align_call(call, n: int, cap: int) -> list:
    """call(out, cigar, cap, used) -> rc, with a cigar buffer of `cap` entries; once more with what was
    needed if that was too small."""
    out = (_Alignment * max(n, 1))()
    used = ctypes.c_longlong(0)
    for _ in range(2):
        cigar = np.zeros(max(cap, 1), dtype=np.uint32)
        rc = call(out, cigar.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), len(cigar), ctypes.byref(used))
        if rc == 0 or used.value <= len(cigar):
            break
        cap = used.value
    _check(rc)
    return _alignments(out[:n], cigar)


# a long call's first guess at the cigar entries: a second call would repeat seconds of device work
_LONG_CIGAR_CAP = 1 << 16


def _align_pairs(f, pairs, matrix, gap_init: int, gap_ext: int, cap: int = 0, mode=None, band=None) -> list:
    """f: one of the library's sw_align_matrix_* entry points over host pairs (mode: a *_mode one; mode
    and band: a *_band one)."""
    if mode is not None and not isinstance(matrix, Matrix):
        raise ValueError("an alignment mode needs a substitution matrix (Matrix.equality gives equality scoring as one)")
    extra = () if mode is None else (int(mode),) if band is None else (int(mode), int(band))
    arrs = [(_u8(a), _u8(b)) for a, b in pairs]
    n = len(arrs)
    if n == 0:
        return []
    u8p = ctypes.POINTER(ctypes.c_ubyte)
    A = (u8p * n)(*[_ptr(x) for x, _ in arrs])
    B = (u8p * n)(*[_ptr(y) for _, y in arrs])
    AL = (ctypes.c_int * n)(*[len(x) for x, _ in arrs])
    BL = (ctypes.c_int * n)(*[len(y) for _, y in arrs])
    return _align_call(lambda out, cig, cap, used: f(matrix._handle(), A, AL, B, BL, n, int(gap_init), int(gap_ext),
                                                     *extra, out, cig, cap, used), n, max(16 * n, cap))


def align_matrix_batch(pairs: Iterable[Sequence], matrix: Matrix, gap_init: int, gap_ext: int, cpu: bool = False,
                       mode: str = "local", long: bool = False, band: int | None = None, coop: bool = False) -> list:
    """An :class:`Alignment` per pair under ``matrix`` (seq1 is its first index) with affine gaps, on
    the GPU (sw_align_matrix_batch: the traced matrix kernel and a walk) or, with ``cpu=True``, from
    the library's plain full-matrix aligner on the host (sw_align_matrix_cpu), which gives the same
    result.  Which alignment is reported when several reach the score is fixed (include/algoGPU.h).
    ``mode``: "local", "global" (both sequences end to end) or "semiglobal" (seq1 end to end inside
    seq2); ``long=True`` is :func:`align_matrix_long` in local mode only (that function takes ``mode=`` itself).
    ``band=B`` (any mode, not with ``long=True``): the alignment within the band of
    :func:`score_matrix_batch`, from the band kernels (sw_align_matrix_batch_band), which hold only the
    band's trace (:func:`band_plan`), or with ``cpu=True`` from the host aligner restricted to it.
    ``coop=True`` (with ``long=True`` only): :func:`align_matrix_long` with ``coop=True``."""
    am = _mode(mode)
    if coop:
        if band is not None:
            raise ValueError("band= is not built for coop=True (the cooperative long path)")
        if not long:
            raise ValueError("coop=True is not built without long=True (it is the checkpointed traceback on many waves)")
    if band is not None:
        if long:
            raise ValueError("band= is not built for long=True (checkpointed traceback)")
        f = lib().sw_align_matrix_cpu_band if cpu else lib().sw_align_matrix_batch_band
        return _align_pairs(f, pairs, matrix, gap_init, gap_ext, mode=am, band=_band(band))
    if long:
        if am != SW_MODE_LOCAL:
            raise ValueError("mode=%r is not built for long=True (checkpointed traceback): it is local only; "
                             "align_matrix_long(..., mode=%r) aligns long pairs in that mode" % (mode, mode))
        if cpu:
            raise ValueError("long=True is a GPU path: not with cpu=True")
        return align_matrix_long(pairs, matrix, gap_init, gap_ext, coop=coop)
    if am != SW_MODE_LOCAL:
        f = lib().sw_align_matrix_cpu_mode if cpu else lib().sw_align_matrix_batch_mode
        return _align_pairs(f, pairs, matrix, gap_init, gap_ext, mode=am)
    return _align_pairs(lib().sw_align_matrix_cpu if cpu else lib().sw_align_matrix_batch, pairs, matrix, gap_init, gap_ext)


def align_matrix_long(pairs: Iterable[Sequence], matrix: Matrix, gap_init: int, gap_ext: int, coop: bool = False,
                      mode: str = "local") -> list:
    """:func:`align_matrix_batch` for pairs whose whole trace does not fit option ``trace_mb``: the same
    alignments, bit for bit, by checkpointed traceback (sw_align_matrix_long): a locate pass keeps the
    right-edge column of every strip of 512 seq1 positions, then the strips are filled again and
    walked one at a time, right to left.  Memory: :func:`align_long_plan`.
    ``coop=True`` (sw_align_matrix_long_coop): the same alignments with the locate pass of a pair on as
    many waves as it has strips and a window of strips filled a round (option ``long_window``), for one or
    a few long pairs.  Memory: :func:`align_long_coop_plan`.
    ``mode`` "global" or "semiglobal" (sw_align_matrix_long_mode, sw_align_matrix_long_coop_mode): the
    alignments of ``align_matrix_batch(..., mode=mode)``, bit for bit, by the same two paths; the plans do
    not depend on the mode."""
    am = _mode(mode)
    if am != SW_MODE_LOCAL:
        f = lib().sw_align_matrix_long_coop_mode if coop else lib().sw_align_matrix_long_mode
        return _align_pairs(f, pairs, matrix, gap_init, gap_ext, _LONG_CIGAR_CAP, mode=am)
    f = lib().sw_align_matrix_long_coop if coop else lib().sw_align_matrix_long
    return _align_pairs(f, pairs, matrix, gap_init, gap_ext, _LONG_CIGAR_CAP)


def align_long_coop_plan(n: int, m: int) -> dict:
    """What ``align_matrix_long(..., coop=True)`` needs for one n x m pair under the current ``trace_mb``,
    SWMI_ALIGN_CKPT_MB and ``long_window`` (sw_align_long_coop_plan, no GPU call): ``strips``, ``ckpt_bytes``,
    ``progress_bytes``, ``end_bytes``, the ``window`` of strips a round would fill for the pair alone and its
    ``window_trace_bytes``.  Raises :class:`SwError` where :func:`align_long_plan` does."""
    p = _AlignCoopPlan()
    _check(lib().sw_align_long_coop_plan(int(n), int(m), ctypes.byref(p)))
    return {"strips": p.strips, "ckpt_bytes": p.ckpt_bytes, "progress_bytes": p.progress_bytes, "end_bytes": p.end_bytes,
            "window": p.window, "window_trace_bytes": p.window_trace_bytes}


def align_long_plan(n: int, m: int) -> dict:
    """What :func:`align_matrix_long` needs for one n x m pair under the current ``trace_mb`` and
    SWMI_ALIGN_CKPT_MB (no GPU call): ``strips``, ``ckpt_bytes``, ``strip_trace_bytes`` and
    ``full_trace_bytes`` (what :func:`align_matrix_batch` would need).  Raises :class:`SwError` when
    the pair would be refused."""
    p = _AlignPlan()
    _check(lib().sw_align_long_plan(int(n), int(m), ctypes.byref(p)))
    return {"strips": p.strips, "ckpt_bytes": p.ckpt_bytes, "strip_trace_bytes": p.strip_trace_bytes,
            "full_trace_bytes": p.full_trace_bytes}


def align_matrix(seq1, seq2, matrix: Matrix, gap_init: int, gap_ext: int, cpu: bool = False, mode: str = "local",
                 long: bool = False, band: int | None = None, coop: bool = False) -> Alignment:
    """One pair (see :func:`align_matrix_batch`)."""
    return align_matrix_batch([(seq1, seq2)], matrix, gap_init, gap_ext, cpu=cpu, mode=mode, long=long, band=band,
                              coop=coop)[0]


def band_plan(n: int, m: int, band: int) -> dict:
    """The band of an n x m pair (sw_band_plan, no GPU call): ``dlo`` and ``dhi`` (a cell (i, j) is in the
    band iff dlo <= j - i <= dhi), ``cells`` in the band, ``trace_bytes`` the traced band launch holds for
    the pair and ``full_trace_bytes`` the unbanded launch would."""
    p = _BandPlan()
    _check(lib().sw_band_plan(int(n), int(m), _band(band), ctypes.byref(p)))
    return {"dlo": p.dlo, "dhi": p.dhi, "cells": p.cells, "trace_bytes": p.trace_bytes,
            "full_trace_bytes": p.full_trace_bytes}


def coop_plan(n: int, m: int, mode: str = "local") -> dict:
    """What ``score_matrix(..., coop=True)`` would choose for one n x m pair under the current options
    (sw_matrix_coop_plan, no GPU call): ``W``, ``strips``, ``swap`` (seq2 across the lanes),
    ``edge_bytes`` and ``items``.  Raises :class:`SwError` when the pair would be refused."""
    p = _CoopPlan()
    _check(lib().sw_matrix_coop_plan(int(n), int(m), _mode(mode), ctypes.byref(p)))
    return {"W": p.W, "strips": p.strips, "swap": p.swap, "edge_bytes": p.edge_bytes, "items": p.items}


# ---- position-specific scoring (include/algoGPU.h sw_profile_*) --------------------------------------

class Profile:
    """A profile: n >= 1 positions over K <= 32 distinct byte symbols, ``scores[i][c]`` what symbol c of the
    sequence scores at position i (a PSSM, a family profile, a query with masked or up-weighted positions).
    ``other`` and ``fold_case`` as for :class:`Matrix`.  The profile is seq1 of every call that takes one: an
    "I" consumes a profile position, ``beg1`` / ``end1`` are profile positions, and in "semiglobal" mode the
    profile is what is covered end to end.  Immutable; usable from any thread."""

    def __init__(self, symbols=None, scores=None, other: int = -1, fold_case: bool = False, _handle=None):
        if _handle is None:
            sym = _u8(symbols)
            tab = np.ascontiguousarray(scores, dtype=np.int64)
            k = len(sym)
            if k == 0 or tab.size % k != 0 or (tab.ndim == 2 and tab.shape[1] != k):
                raise SwError("profile: the table is not n x %d" % k)
            n = tab.size // k
            if tab.size and (tab.min() < -127 or tab.max() > 127):
                raise SwError("profile: an entry is outside [-127, 127]")
            t8 = tab.reshape(-1).astype(np.int8)
            _handle = lib().sw_profile_create(_ptr(sym), k, t8.ctypes.data_as(ctypes.POINTER(ctypes.c_byte)), n,
                                              int(other), SW_MATRIX_FOLD_CASE if fold_case else 0)
        if not _handle:
            raise SwError(lib().sw_last_error().decode(errors="replace"))
        self._h = ctypes.c_void_p(_handle)

    @classmethod
    def parse(cls, text) -> "Profile":
        """From the library's own text format: '#' comment lines, a header line of K symbols, then a row a
        position: a one-byte label (the consensus residue, ignored) and K integers."""
        if isinstance(text, str):
            text = text.encode("latin-1")
        return cls(_handle=lib().sw_profile_parse(text, len(text)) or 0)

    @classmethod
    def open(cls, path) -> "Profile":
        return cls(_handle=lib().sw_profile_open(os.fsencode(path)) or 0)

    @classmethod
    def from_matrix(cls, matrix: Matrix, query) -> "Profile":
        """Row i is ``matrix``'s row of query byte i: the profile calls then give what the matrix calls give
        with ``query`` as seq1."""
        q = _u8(query)
        return cls(_handle=lib().sw_profile_from_matrix(matrix._handle(), _ptr(q), len(q)) or 0)

    def _handle(self):
        if self._h is None:
            raise SwError("profile is closed")
        return self._h

    def __len__(self) -> int:
        return lib().sw_profile_length(self._handle())

    @property
    def symbols(self) -> bytes:
        k = lib().sw_profile_size(self._handle())
        out = np.zeros(max(k, 1), dtype=np.uint8)
        _check(lib().sw_profile_symbols(self._handle(), _ptr(out)))
        return out[:k].tobytes()

    def score(self, pos: int, byte) -> int:
        """The entry of position ``pos`` for ``byte``, through the byte-to-code map the kernel uses."""
        out = ctypes.c_int()
        _check(lib().sw_profile_score(self._handle(), int(pos), int(_u8(byte)[0]), ctypes.byref(out)))
        return out.value

    def close(self) -> None:
        if self._h is not None and self._h.value:
            lib().sw_profile_free(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _seq_arrays(seqs):
    arrs = [_u8(x) for x in seqs]
    n = len(arrs)
    u8p = ctypes.POINTER(ctypes.c_ubyte)
    return arrs, (u8p * n)(*[_ptr(x) for x in arrs]), (ctypes.c_int * n)(*[len(x) for x in arrs])


def score_profile_batch(profile: Profile, seqs: Iterable, gap_init: int, gap_ext: int, mode: str = "local") -> list:
    """The score of ``profile`` (seq1) against every sequence of ``seqs`` in one launch
    (sw_score_profile_batch): the recurrence of :func:`score_matrix_batch` in ``mode``, with the score of a
    cell read from the profile's row of its position.  No ``band=``, ``coop=`` or long path with a profile."""
    am = _mode(mode)
    arrs, S, SL = _seq_arrays(seqs)
    n = len(arrs)
    if n == 0:
        return []
    out = (ctypes.c_int * n)()
    _check(lib().sw_score_profile_batch(profile._handle(), S, SL, n, int(gap_init), int(gap_ext), am, out))
    return list(out)


def score_profile(profile: Profile, seq, gap_init: int, gap_ext: int, mode: str = "local") -> int:
    """One sequence (see :func:`score_profile_batch`)."""
    return score_profile_batch(profile, [seq], gap_init, gap_ext, mode=mode)[0]


def align_profile_batch(profile: Profile, seqs: Iterable, gap_init: int, gap_ext: int, cpu: bool = False,
                        mode: str = "local") -> list:
    """An :class:`Alignment` of ``profile`` (seq1) with every sequence of ``seqs``, on the GPU
    (sw_align_profile_batch) or, with ``cpu=True``, from the library's host aligner (sw_align_profile_cpu),
    which gives the same result bit for bit.  End cell, walk and modes as :func:`align_matrix_batch`."""
    am = _mode(mode)
    arrs, S, SL = _seq_arrays(seqs)
    n = len(arrs)
    if n == 0:
        return []
    f = lib().sw_align_profile_cpu if cpu else lib().sw_align_profile_batch
    return _align_call(lambda out, cig, cap, used: f(profile._handle(), S, SL, n, int(gap_init), int(gap_ext), am, out, cig,
                                                     cap, used), n, 16 * n)


def align_profile(profile: Profile, seq, gap_init: int, gap_ext: int, cpu: bool = False, mode: str = "local") -> Alignment:
    """One sequence (see :func:`align_profile_batch`)."""
    return align_profile_batch(profile, [seq], gap_init, gap_ext, cpu=cpu, mode=mode)[0]


# ---- translated search: protein queries against DNA in six reading frames (include/algoGPU.h sw_*_translated*) ----

FRAMES = (1, 2, 3, -1, -2, -3)
STANDARD_CODE = b"FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"


def _code(code):
    """``code`` as the library takes it: None (the standard code), or 64 bytes in NCBI's TCAG order."""
    if code is None:
        return None, None
    c = _u8(code)
    if len(c) != 64:
        raise ValueError("a genetic code is 64 bytes, one amino acid a codon in TCAG order (got %d)" % len(c))
    return c, _ptr(c)


def _frame(frame) -> int:
    if isinstance(frame, bool) or not isinstance(frame, (int, np.integer)) or int(frame) not in FRAMES:
        raise ValueError("frame %r is not one of +1, +2, +3, -1, -2, -3" % (frame,))
    return int(frame)


def translate(dna, frame: int, code=None) -> bytes:
    """Reading frame ``frame`` (+1, +2, +3, -1, -2, -3) of ``dna`` as protein under ``code`` (64 bytes in TCAG order;
    None: the standard code), by the rules the translated kernels follow (sw_translate): T/U, C, A, G in either
    case, any codon with another byte is ``X`` (degenerate codons are not resolved), stops are ``*``.  A minus frame
    reads the reverse complement; translating a DNA *query* into its six frames and searching a protein database
    with each is the other direction (blastx)."""
    d = _u8(dna)
    keep, cp = _code(code)
    out = np.zeros(len(d) // 3 + 1, dtype=np.uint8)
    m = _check(lib().sw_translate(_ptr(d), len(d), _frame(frame), cp, _ptr(out), len(out)))
    return out[:m].tobytes()


def translated_range(length: int, frame: int, beg2: int, end2: int) -> tuple:
    """The half-open DNA range, forward strand, that residues [beg2, end2) of ``frame`` of a DNA of ``length`` bases
    cover (sw_translated_range)."""
    b, e = ctypes.c_int(), ctypes.c_int()
    _check(lib().sw_translated_range(int(length), _frame(frame), int(beg2), int(end2), ctypes.byref(b), ctypes.byref(e)))
    return b.value, e.value


@dataclass(frozen=True)
class TranslatedAlignment(Alignment):
    """An :class:`Alignment` of a protein (seq1) with one reading frame of a DNA (seq2): ``beg2`` / ``end2`` are
    residues of ``frame``, and [``dna_beg``, ``dna_end``) is the range of bases they cover on the forward strand.
    ``columns(query, translate(dna, frame))`` gives the aligned rows."""
    frame: int = 1
    dna_beg: int = 0
    dna_end: int = 0


def score_matrix_translated_batch(pairs: Iterable[Sequence], matrix: Matrix, gap_init: int, gap_ext: int, mode: str = "local",
                                  code=None) -> np.ndarray:
    """int32 scores, shape (npairs, 6): the protein of every (protein, dna) pair against the six reading frames of
    its DNA, frames +1, +2, +3, -1, -2, -3 in this order, in one launch (sw_score_matrix_translated_batch).  The
    kernel translates as it fetches; entry [k, f] equals ``score_matrix(protein, translate(dna, FRAMES[f], code),
    ...)``.  The matrix must score every byte the code can emit, ``*`` and ``X`` among them.  No ``band=``,
    ``coop=``, long path or profile against a translated frame."""
    am = _mode(mode)
    keep, cp = _code(code)
    arrs = [(_u8(a), _u8(b)) for a, b in pairs]
    n = len(arrs)
    out = np.zeros((n, 6), dtype=np.int32)
    if n == 0:
        return out
    u8p = ctypes.POINTER(ctypes.c_ubyte)
    A = (u8p * n)(*[_ptr(x) for x, _ in arrs])
    B = (u8p * n)(*[_ptr(y) for _, y in arrs])
    AL = (ctypes.c_int * n)(*[len(x) for x, _ in arrs])
    BL = (ctypes.c_int * n)(*[len(y) for _, y in arrs])
    _check(lib().sw_score_matrix_translated_batch(matrix._handle(), A, AL, B, BL, n, int(gap_init), int(gap_ext), am, cp,
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    return out


def score_matrix_translated(protein, dna, matrix: Matrix, gap_init: int, gap_ext: int, mode: str = "local",
                            code=None) -> np.ndarray:
    """One pair (see :func:`score_matrix_translated_batch`): the six scores."""
    return score_matrix_translated_batch([(protein, dna)], matrix, gap_init, gap_ext, mode=mode, code=code)[0]


def _translated(als, frames, dlens) -> list:
    """TranslatedAlignment of every Alignment with its frame and the DNA range of [beg2, end2)."""
    res = []
    for x, f, L in zip(als, frames, dlens):
        b, e = translated_range(L, f, x.beg2, x.end2)
        res.append(TranslatedAlignment(x.score, x.beg1, x.end1, x.beg2, x.end2, x.ops, f, b, e))
    return res


def align_matrix_translated_batch(pairs: Iterable[Sequence], frames, matrix: Matrix, gap_init: int, gap_ext: int,
                                  cpu: bool = False, mode: str = "local", code=None) -> list:
    """A :class:`TranslatedAlignment` per (protein, dna) pair in the frame ``frames[k]`` names, on the GPU
    (sw_align_matrix_translated_batch: the traced translated kernel and the matrix path's walk) or, with
    ``cpu=True``, from the host (sw_align_matrix_translated_cpu: translate, then the host aligner), which gives the
    same result bit for bit.  A pair whose trace does not fit option ``trace_mb`` is refused: there is no long
    path, band or cooperative path against a translated frame."""
    am = _mode(mode)
    keep, cp = _code(code)
    arrs = [(_u8(a), _u8(b)) for a, b in pairs]
    fr = [_frame(f) for f in frames]
    n = len(arrs)
    if len(fr) != n:
        raise ValueError("%d frames for %d pairs" % (len(fr), n))
    if n == 0:
        return []
    u8p = ctypes.POINTER(ctypes.c_ubyte)
    A = (u8p * n)(*[_ptr(x) for x, _ in arrs])
    B = (u8p * n)(*[_ptr(y) for _, y in arrs])
    AL = (ctypes.c_int * n)(*[len(x) for x, _ in arrs])
    BL = (ctypes.c_int * n)(*[len(y) for _, y in arrs])
    FR = (ctypes.c_int * n)(*fr)
    f = lib().sw_align_matrix_translated_cpu if cpu else lib().sw_align_matrix_translated_batch
    als = _align_call(lambda out, cig, cap, used: f(matrix._handle(), A, AL, B, BL, FR, n, int(gap_init), int(gap_ext), am, cp,
                                                    out, cig, cap, used), n, 16 * n)
    return _translated(als, fr, [len(y) for _, y in arrs])


def align_matrix_translated(protein, dna, frame: int, matrix: Matrix, gap_init: int, gap_ext: int, cpu: bool = False,
                            mode: str = "local", code=None) -> TranslatedAlignment:
    """One pair (see :func:`align_matrix_translated_batch`)."""
    return align_matrix_translated_batch([(protein, dna)], [frame], matrix, gap_init, gap_ext, cpu=cpu, mode=mode, code=code)[0]


def last_align_ms() -> tuple:
    """(fill_ms, walk_ms): device time of this thread's last GPU alignment call, over its launches."""
    f, w = ctypes.c_float(), ctypes.c_float()
    lib().sw_last_align_ms(ctypes.byref(f), ctypes.byref(w))
    return f.value, w.value


def last_align_long_ms() -> dict:
    """Device time of this thread's last :func:`align_matrix_long` / ``Database.align(long=True)`` call
    (with or without ``coop=True``): ``locate_ms``, ``strip_ms`` (the strip fills), ``walk_ms``, and its ``rounds``."""
    lo, st, wk, r = ctypes.c_float(), ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
    lib().sw_last_align_long_ms(ctypes.byref(lo), ctypes.byref(st), ctypes.byref(wk), ctypes.byref(r))
    return {"locate_ms": lo.value, "strip_ms": st.value, "walk_ms": wk.value, "rounds": r.value}


from .db import Database  # noqa: E402  (FASTA databases, query x database search)
