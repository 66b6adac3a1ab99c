"""FASTA databases and query x database search.

The reference drives database search only through the external CUDASW++4 tool
(timing.sh:3-8: ``makedb SwissProt.fasta benchdb/sp`` then
``align --query q.fa --db benchdb/sp``).  This is the same workflow over the
engine's C-ABI (include/algoGPU.h ``sw_db_*``): the parse, the database file
and the search all run in libswmi355.so; a search is one batch launch over
residues resident in HBM.  Scores are the reference's byte-equality affine
scores (main.cpp:28-66), so ``Database.search(q)[i]`` equals
``SmithWatermanScore(q, record i)``; with ``matrix=`` (a ``Matrix`` read from a
file such as BLOSUM62) they are substitution-matrix scores.

    db = Database.open("sp.fasta")          # or a file written by db.save()
    scores = db.search(b"MKTAYIAKQR...")    # one int per record, record order
    db.top(b"MKTAYIAKQR...", k=10)          # [(score, index, header), ...]
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import FRAMES, _LONG_CIGAR_CAP, SwError, _align_call, _check, _code, _frame, _mode, _ptr, _translated, _u8, lib


class Database:
    """A handle on an ``sw_db`` (records + their residues, host and HBM)."""

    def __init__(self, handle: int):
        if not handle:
            raise SwError(lib().sw_last_error().decode(errors="replace"))
        self._h = ctypes.c_void_p(handle)

    # ---- construction -------------------------------------------------------
    @classmethod
    def open(cls, path: str | os.PathLike) -> "Database":
        """A FASTA file or a database file written by :meth:`save`."""
        return cls(lib().sw_db_open(os.fsencode(path)))

    @classmethod
    def from_fasta(cls, text: bytes | str) -> "Database":
        if isinstance(text, str):
            text = text.encode("latin-1")
        return cls(lib().sw_db_from_fasta(text, len(text)))

    @classmethod
    def from_records(cls, records) -> "Database":
        """From (header, sequence) pairs; headers must not contain a line end."""
        parts = []
        for h, s in records:
            h = h.encode("latin-1") if isinstance(h, str) else bytes(h)
            parts.append(b">" + h + b"\n" + _u8(s).tobytes() + b"\n")
        return cls.from_fasta(b"".join(parts))

    def save(self, path: str | os.PathLike) -> None:
        """The binary database file (the ``makedb`` step)."""
        _check(lib().sw_db_save(self._h, os.fsencode(path)))

    def close(self) -> None:
        if self._h is not None and self._h.value:
            lib().sw_db_close(self._h)
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

    # ---- records --------------------------------------------------------------
    def __len__(self) -> int:
        return lib().sw_db_count(self._h)

    @property
    def residues(self) -> int:
        return lib().sw_db_residues(self._h)

    def record(self, i: int) -> tuple:
        """(header, residues as bytes) of record i."""
        seq = ctypes.POINTER(ctypes.c_ubyte)()
        n = ctypes.c_int()
        hdr = ctypes.c_char_p()
        _check(lib().sw_db_record(self._h, int(i), ctypes.byref(seq), ctypes.byref(n), ctypes.byref(hdr)))
        return hdr.value.decode("latin-1"), ctypes.string_at(seq, n.value) if n.value else b""

    def length(self, i: int) -> int:
        """Residues of record i (no copy: sw_db_record with seq = NULL)."""
        n = ctypes.c_int()
        _check(lib().sw_db_record(self._h, int(i), None, ctypes.byref(n), None))
        return n.value

    def header(self, i: int) -> str:
        """Header of record i (no residue copy)."""
        hdr = ctypes.c_char_p()
        _check(lib().sw_db_record(self._h, int(i), None, None, ctypes.byref(hdr)))
        return hdr.value.decode("latin-1")

    def lengths(self) -> np.ndarray:
        return np.array([self.length(i) for i in range(len(self))], dtype=np.int64)

    # ---- search ---------------------------------------------------------------
    @staticmethod
    def _gaps(matrix, gap_init, gap_ext):
        if matrix is None:
            if gap_init is not None or gap_ext is not None:
                raise SwError("gap_init / gap_ext go with matrix= (equality searches use set_params)")
            return None
        if gap_init is None or gap_ext is None:
            raise SwError("a matrix search needs gap_init and gap_ext")
        return int(gap_init), int(gap_ext)

    @staticmethod
    def _amode(mode, matrix, what=None):
        """SW_MODE_* of ``mode``; a non-local mode needs a matrix and is not built for ``what``."""
        am = _mode(mode)
        if am != 0 and what:
            raise ValueError("mode=%r is not built for %s: it is local only%s" % (
                mode, what, "; Database.align_long(..., mode=%r) aligns long records in that mode" % (mode,)
                if what.startswith("long=True") else ""))
        if am != 0 and matrix is None:
            raise ValueError("mode=%r needs matrix= (Matrix.equality gives the table of an equality scoring)" % (mode,))
        return am

    def search(self, query, matrix=None, gap_init=None, gap_ext=None, mode: str = "local") -> np.ndarray:
        """int32 score of ``query`` against every record, in record order.  With ``matrix`` (a
        :class:`Matrix`; the query is its first index) the scores are substitution-matrix scores
        with the gap penalties given here; without, byte-equality scores as set_params has them.
        ``mode`` (matrix searches): "local"; "semiglobal", the whole query inside the record, the
        record's flanks free; "global", query and record end to end.  Scores of the last two may
        be negative."""
        q = _u8(query)
        out = np.zeros(len(self), dtype=np.int32)
        am = self._amode(mode, matrix)
        gaps = self._gaps(matrix, gap_init, gap_ext)
        if gaps is not None and am != 0:
            _check(lib().sw_db_search_matrix_mode(self._h, matrix._handle(), _ptr(q), len(q), gaps[0], gaps[1], am,
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
            return out
        if gaps is not None:
            _check(lib().sw_db_search_matrix(self._h, matrix._handle(), _ptr(q), len(q), gaps[0], gaps[1],
                                             out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
            return out
        _check(lib().sw_db_search(self._h, _ptr(q), len(q), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    def search_db(self, queries: "Database", matrix=None, gap_init=None, gap_ext=None, mode: str = "local") -> np.ndarray:
        """[len(queries), len(self)] int32 scores of every query record against every record
        (``matrix``, ``gap_init``, ``gap_ext`` as in :meth:`search`; matrix queries run one by one).
        Local only: any other ``mode`` raises ValueError."""
        self._amode(mode, matrix, "search_db")
        out = np.zeros((len(queries), len(self)), dtype=np.int32)
        gaps = self._gaps(matrix, gap_init, gap_ext)
        if gaps is not None:
            _check(lib().sw_db_search_db_matrix(self._h, queries._h, matrix._handle(), gaps[0], gaps[1],
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
            return out
        _check(lib().sw_db_search_db(self._h, queries._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    def align(self, query, indices, matrix, gap_init: int, gap_ext: int, long: bool = False, mode: str = "local",
              coop: bool = False) -> list:
        """An :class:`Alignment` of ``query`` (seq1) with each record of ``indices``, out of the
        database's device arena (sw_db_align_matrix): only the query is uploaded.  ``long=True``: the
        same alignments by checkpointed traceback (sw_db_align_matrix_long), for records whose whole
        trace does not fit option ``trace_mb`` (local only: :meth:`align_long` takes a mode); with ``coop=True`` as well, on many waves
        (sw_db_align_matrix_long_coop: ``align_matrix_long(..., coop=True)``).  ``mode`` as in :meth:`search`."""
        if coop and not long:
            raise ValueError("coop=True is not built without long=True (it is the checkpointed traceback on many waves)")
        am = self._amode(mode, matrix, "long=True (checkpointed traceback)" if long else None)
        q = _u8(query)
        idx = [int(i) for i in indices]
        n = len(idx)
        if n == 0:
            return []
        IDX = (ctypes.c_int * n)(*idx)
        if am != 0:
            return _align_call(lambda out, cig, cap, used: lib().sw_db_align_matrix_mode(
                self._h, matrix._handle(), _ptr(q), len(q), IDX, n, int(gap_init), int(gap_ext), am, out, cig, cap, used), n,
                16 * n)
        f = lib().sw_db_align_matrix_long_coop if coop else lib().sw_db_align_matrix_long if long else lib().sw_db_align_matrix
        return _align_call(lambda out, cig, cap, used: f(
            self._h, matrix._handle(), _ptr(q), len(q), IDX, n, int(gap_init), int(gap_ext), out, cig, cap, used), n,
            max(16 * n, _LONG_CIGAR_CAP if long else 0))

    def align_long(self, query, indices, matrix, gap_init: int, gap_ext: int, mode: str = "local", coop: bool = False) -> list:
        """:meth:`align` with ``long=True`` in any ``mode``: checkpointed traceback of ``query`` (seq1) with each
        record of ``indices`` (sw_db_align_matrix_long_mode; with ``coop=True`` on many waves,
        sw_db_align_matrix_long_coop_mode).  Global and semi-global alignments are those of
        ``align(..., mode=mode)``, bit for bit, for records whose whole trace does not fit option ``trace_mb``;
        ``mode="local"`` is ``align(..., long=True, coop=coop)``."""
        am = self._amode(mode, matrix)
        if am == 0:
            return self.align(query, indices, matrix, gap_init, gap_ext, long=True, coop=coop)
        q = _u8(query)
        idx = [int(i) for i in indices]
        n = len(idx)
        if n == 0:
            return []
        IDX = (ctypes.c_int * n)(*idx)
        f = lib().sw_db_align_matrix_long_coop_mode if coop else lib().sw_db_align_matrix_long_mode
        return _align_call(lambda out, cig, cap, used: f(
            self._h, matrix._handle(), _ptr(q), len(q), IDX, n, int(gap_init), int(gap_ext), am, out, cig, cap, used), n,
            max(16 * n, _LONG_CIGAR_CAP))

    # ---- profiles (position-specific scoring: concurrentproject_amd.Profile) ----------------------
    def search_profile(self, profile, gap_init: int, gap_ext: int, mode: str = "local") -> np.ndarray:
        """int32 score of ``profile`` (seq1) against every record, in record order (sw_db_search_profile);
        ``mode`` as in :meth:`search`.  The records are checked against the profile's alphabet once."""
        out = np.zeros(len(self), dtype=np.int32)
        _check(lib().sw_db_search_profile(self._h, profile._handle(), int(gap_init), int(gap_ext), _mode(mode),
                                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    def align_profile(self, profile, indices, gap_init: int, gap_ext: int, mode: str = "local") -> list:
        """An :class:`Alignment` of ``profile`` (seq1) with each record of ``indices``, out of the database's
        device arena (sw_db_align_profile)."""
        am = _mode(mode)
        idx = [int(i) for i in indices]
        n = len(idx)
        if n == 0:
            return []
        IDX = (ctypes.c_int * n)(*idx)
        return _align_call(lambda out, cig, cap, used: lib().sw_db_align_profile(
            self._h, profile._handle(), IDX, n, int(gap_init), int(gap_ext), am, out, cig, cap, used), n, 16 * n)

    def top_profile(self, profile, k: int = 10, gap_init: int = 0, gap_ext: int = 0, alignments: bool = False,
                    mode: str = "local") -> list:
        """:meth:`top` for a profile: the k best records as [(score, index, header)], score descending, index
        ascending on ties; with ``alignments=True`` each tuple ends with the hit's :class:`Alignment`."""
        sc = self.search_profile(profile, gap_init, gap_ext, mode=mode)
        idx = np.lexsort((np.arange(len(sc)), -sc.astype(np.int64)))[:k]
        hits = [(int(sc[i]), int(i), self.header(int(i))) for i in idx]
        if not alignments:
            return hits
        al = self.align_profile(profile, [h[1] for h in hits], gap_init, gap_ext, mode=mode)
        return [h + (x,) for h, x in zip(hits, al)]

    # ---- translated search: a protein query against DNA records in six reading frames ---------------
    def search_translated(self, query, matrix, gap_init: int, gap_ext: int, mode: str = "local", code=None) -> np.ndarray:
        """int32 scores, shape (len(self), 6): the protein ``query`` against the six reading frames (+1, +2, +3, -1,
        -2, -3) of every DNA record, translated by the kernel as it reads the arena (sw_db_search_matrix_translated);
        ``code``: a genetic code of 64 bytes (None: the standard one).  The records are not checked against the
        matrix: any byte is a DNA byte, and a codon with a byte other than T/U, C, A, G is ``X``."""
        q = _u8(query)
        keep, cp = _code(code)
        out = np.zeros((len(self), 6), dtype=np.int32)
        _check(lib().sw_db_search_matrix_translated(self._h, matrix._handle(), _ptr(q), len(q), int(gap_init), int(gap_ext),
                                                    _mode(mode), cp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    def align_translated(self, query, indices, frames, matrix, gap_init: int, gap_ext: int, mode: str = "local",
                         code=None) -> list:
        """A :class:`TranslatedAlignment` of ``query`` (seq1) with frame ``frames[k]`` of record ``indices[k]``, out of
        the database's device arena (sw_db_align_matrix_translated)."""
        am = _mode(mode)
        q = _u8(query)
        keep, cp = _code(code)
        idx = [int(i) for i in indices]
        fr = [_frame(f) for f in frames]
        n = len(idx)
        if len(fr) != n:
            raise ValueError("%d frames for %d records" % (len(fr), n))
        if n == 0:
            return []
        IDX = (ctypes.c_int * n)(*idx)
        FR = (ctypes.c_int * n)(*fr)
        als = _align_call(lambda out, cig, cap, used: lib().sw_db_align_matrix_translated(
            self._h, matrix._handle(), _ptr(q), len(q), IDX, FR, n, int(gap_init), int(gap_ext), am, cp, out, cig, cap, used),
            n, 16 * n)
        return _translated(als, fr, [self.length(i) for i in idx])

    def top_translated(self, query, k: int = 10, matrix=None, gap_init: int = 0, gap_ext: int = 0, alignments: bool = False,
                       mode: str = "local", code=None) -> list:
        """The k best (record, frame) hits of :meth:`search_translated`: [(score, index, frame, header)], score
        descending, then index ascending, then frame order +1, +2, +3, -1, -2, -3; with ``alignments=True`` each
        tuple ends with the hit's :class:`TranslatedAlignment`."""
        sc = self.search_translated(query, matrix, gap_init, gap_ext, mode=mode, code=code).reshape(-1)
        flat = np.lexsort((np.arange(len(sc)), -sc.astype(np.int64)))[:k]   # flat = 6 * index + frame index
        hits = [(int(sc[i]), int(i) // 6, FRAMES[int(i) % 6], self.header(int(i) // 6)) for i in flat]
        if not alignments:
            return hits
        al = self.align_translated(query, [h[1] for h in hits], [h[2] for h in hits], matrix, gap_init, gap_ext, mode=mode,
                                   code=code)
        return [h + (x,) for h, x in zip(hits, al)]

    def top(self, query, k: int = 10, matrix=None, gap_init=None, gap_ext=None, alignments: bool = False,
            mode: str = "local") -> list:
        """The k best records: [(score, index, header)], score descending, index ascending on ties.
        With ``alignments=True`` (a matrix search) each tuple ends with the hit's :class:`Alignment`.
        ``mode`` as in :meth:`search`; the ranking is by score as ever, and scores may be negative."""
        sc = self.search(query, matrix=matrix, gap_init=gap_init, gap_ext=gap_ext, mode=mode)
        idx = np.lexsort((np.arange(len(sc)), -sc.astype(np.int64)))[:k]
        hits = [(int(sc[i]), int(i), self.header(int(i))) for i in idx]
        if not alignments:
            return hits
        if matrix is None:
            raise SwError("alignments=True needs matrix= (Matrix.equality gives the table of an equality scoring)")
        al = self.align(query, [h[1] for h in hits], matrix, gap_init, gap_ext, mode=mode)
        return [h + (x,) for h, x in zip(hits, al)]
