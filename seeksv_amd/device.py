"""Python face of libseeksv_hip.so (include/seeksv_hip.h).  Thin ctypes plumbing: every operation runs in
hand-written HIP kernels on the GPU.  There is no fallback - without the built library or without a GPU
the constructor raises.
"""
import ctypes as C

import numpy as np

from . import _abi
from .host import concat_tables, host_tid_runs, table_to_dict


class SeeksvError(RuntimeError):
    pass


class Context:
    """One GPU, one HIP stream (ssv_ctx)."""

    def __init__(self, device=0):
        self._lib = _abi.hip_lib()
        h = C.c_void_p()
        rc = self._lib.ssv_ctx_create(device, C.byref(h))
        if rc != 0:
            raise SeeksvError(f"ssv_ctx_create({device}) failed ({rc}): {self._lib.ssv_last_error(None).decode()}")
        self._h = h
        self.device = device

    def _check(self, rc, what):
        if rc != 0:
            raise SeeksvError(f"{what} failed ({rc}): {self._lib.ssv_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ssv_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(self._lib.ssv_sync(self._h), "ssv_sync")

    def prefetch(self, batch):
        """announce a host batch (an _abi.Batch over arrays that stay alive - best page-locked, see PinnedArrays): its copy to HBM starts on
        the upload stream now; the next scan call must be given this batch"""
        self._check(self._lib.ssv_batch_prefetch(self._h, C.byref(batch)), "ssv_batch_prefetch")

    def prefetch_drop(self):
        """give up the announced batches (their host arrays may be reused when this returns)"""
        self._check(self._lib.ssv_batch_prefetch_drop(self._h), "ssv_batch_prefetch_drop")

    @staticmethod
    def _as_batch(b):
        if isinstance(b, _abi.Batch):
            return b, None
        return _abi.make_batch(b)

    @staticmethod
    def _as_names(names):
        """an _abi.Names as it is, or one over host memory for a list of names (str or bytes); -> (Names, keepalive)"""
        if isinstance(names, _abi.Names):
            return names, None
        raw = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
        blob = b"".join(x + b"\0" for x in raw)
        off = np.zeros(len(raw) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) + 1 for x in raw])
        buf = C.create_string_buffer(blob, len(blob) + 1)
        return _abi.Names(_abi.MEM_HOST, 0, 0, C.cast(buf, C.c_void_p), off.ctypes.data, len(blob)), (buf, off)

    # ---- getsv -F: junctions from read-through split alignments (ssv_rt_*) ----
    def readthrough(self, batches, names, min_mapq=1, target_names=(), raw=False):
        """FindJunction (process_bwasw.cpp:5-227) over host batches in file order.  batches: dicts of arrays (or _abi.Batch) that carry every kept
        record's bases; names[k]: the read names of batch k (str).  Returns one dict per pair, in the order of the record that completed it:
        the junction (contig names when target_names is given, else tids), microhomology, kind, the two seqs and CIGAR sources with their edits."""
        self.rt_begin(min_mapq, target_names)
        for b, nm in zip(batches, names):
            self.rt_scan(b, nm)
        r = self.rt_finish()
        out = self.rt_decode(r, target_names)
        return (out, r.n_candidates) if raw else out

    def readthrough_original(self, batches, names, min_mapq=1, target_names=(), raw=False):
        """readthrough() under the split-read rule of `run -A` (ssv_rt_begin_original, include/seeksv_hip.h): the batches are an aligner's output in
        input order - primary + supplementary records, hard clips allowed, pairs keyed by (name, flag & 0xC0).  Same rows as readthrough();
        raw: (rows, rt_original_stats())."""
        self.rt_begin_original(min_mapq, target_names)
        for b, nm in zip(batches, names):
            self.rt_scan(b, nm)
        out = self.rt_decode(self.rt_finish(), target_names)
        return (out, self.rt_original_stats()) if raw else out

    def rt_begin_original(self, min_mapq=1, target_names=()):
        """ssv_rt_begin_original: rt_begin() for a session under the split-read rule; rt_scan / rt_finish / rt_decode as they are"""
        self.rt_begin(min_mapq, target_names, _call="ssv_rt_begin_original")

    def rt_original_stats(self):
        """ssv_rt_original_stats: the counts of the last finished rt_begin_original session, a dict of the struct's fields"""
        s = _abi.RtOriginalCounts()
        self._check(self._lib.ssv_rt_original_stats(self._h, C.byref(s)), "ssv_rt_original_stats")
        return {k: int(getattr(s, k)) for k, _ in s._fields_}

    # ---- run -A -S: virtual candidates from SA tags (ssv_rt_begin_original_sa) ----
    def readthrough_original_sa(self, batches, names, auxes, min_mapq=1, target_names=(), raw=False):
        """readthrough_original() with virtual candidates from the SA tag of a source whose partner is absent (ssv_rt_begin_original_sa,
        include/seeksv_hip.h).  auxes[k]: batch k's optional fields - an _abi.Aux, or (encoding, [bytes per record]).  Same rows;
        raw: (rows, rt_original_stats(), rt_original_sa_stats())."""
        self.rt_begin_original_sa(min_mapq, target_names)
        for b, nm, ax in zip(batches, names, auxes):
            self.rt_scan_aux(b, nm, ax)
        out = self.rt_decode(self.rt_finish(), target_names)
        return (out, self.rt_original_stats(), self.rt_original_sa_stats()) if raw else out

    def rt_begin_original_sa(self, min_mapq=1, target_names=()):
        """ssv_rt_begin_original_sa: rt_begin_original() plus the contig names the SA entries are looked up in; batches go through rt_scan_aux"""
        nt = len(target_names)
        raw = [x.encode() if isinstance(x, str) else bytes(x) for x in target_names]
        order = sorted(range(nt), key=lambda t: raw[t])
        rank = np.zeros(max(nt, 1), dtype=np.int32)
        rank[order] = np.arange(nt, dtype=np.int32)
        arr = (C.c_char_p * max(1, nt))(*raw)
        p = _abi.RtParams(int(min_mapq), nt, rank.ctypes.data_as(C.POINTER(C.c_int32)))
        self._check(self._lib.ssv_rt_begin_original_sa(self._h, C.byref(p), arr), "ssv_rt_begin_original_sa")

    @staticmethod
    def _as_aux(aux):
        """an _abi.Aux as it is, or one over host memory for (encoding, [the optional-field bytes of every record]); -> (Aux, keepalive)"""
        if isinstance(aux, _abi.Aux):
            return aux, None
        enc, areas = aux
        blob = b"".join(areas)
        lens = np.array([len(a) for a in areas], dtype=np.uint32)
        off = np.zeros(len(areas) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens, dtype=np.uint64)
        buf = C.create_string_buffer(blob, max(1, len(blob)))
        return _abi.Aux(_abi.MEM_HOST, int(enc), len(areas), C.cast(buf, C.c_void_p), off.ctypes.data, lens.ctypes.data, len(blob)), (buf, off, lens)

    def rt_scan_aux(self, batch, names, aux):
        """ssv_rt_scan_aux: rt_scan() in a session of rt_begin_original_sa.  aux: bamdec_aux() / samdec_aux() for a batch of a device decoder, or
        (encoding, [bytes per record])"""
        bb, keep = self._as_batch(batch)
        n, keep_names = self._as_names(names)
        a, keep_aux = self._as_aux(aux)
        self._check(self._lib.ssv_rt_scan_aux(self._h, C.byref(bb), C.byref(n), C.byref(a)), "ssv_rt_scan_aux")

    def rt_original_sa_stats(self):
        """ssv_rt_original_sa_stats: the seven SA counts of the last finished rt_begin_original_sa session, a dict of the struct's fields"""
        s = _abi.RtOriginalSaCounts()
        self._check(self._lib.ssv_rt_original_sa_stats(self._h, C.byref(s)), "ssv_rt_original_sa_stats")
        return {k: int(getattr(s, k)) for k, _ in s._fields_}

    def bamdec_aux(self):
        """ssv_bamdec_aux: where the optional fields of the batch bam_batches handed out last lie in HBM (valid as long as that batch)"""
        a = _abi.Aux()
        self._check(self._lib.ssv_bamdec_aux(self._h, C.byref(a)), "ssv_bamdec_aux")
        return a

    def samdec_aux(self):
        """ssv_samdec_aux: where the optional fields of the batch decoded last lie in HBM (valid as long as that batch)"""
        a = _abi.Aux()
        self._check(self._lib.ssv_samdec_aux(self._h, C.byref(a)), "ssv_samdec_aux")
        return a

    def rt_begin(self, min_mapq=1, target_names=(), _call="ssv_rt_begin"):
        """ssv_rt_begin: a new -F file; target_names give the contigs' byte-wise name order (and the number of contigs a tid may name)"""
        nt = len(target_names)
        order = sorted(range(nt), key=lambda t: target_names[t].encode())
        rank = np.zeros(max(nt, 1), dtype=np.int32)
        for k, t in enumerate(order):
            rank[t] = k
        p = _abi.RtParams(int(min_mapq), nt, rank.ctypes.data_as(C.POINTER(C.c_int32)))
        self._check(getattr(self._lib, _call)(self._h, C.byref(p)), _call)

    def rt_scan(self, batch, names):
        """ssv_rt_scan: the next batch in file order.  names: the batch's read names (list of str), or an _abi.Names that says where they lie -
        bamdec_names() for a batch of the device decoder"""
        bb, keep = self._as_batch(batch)
        n, keep_names = self._as_names(names)
        self._check(self._lib.ssv_rt_scan(self._h, C.byref(bb), C.byref(n)), "ssv_rt_scan")

    def rt_finish(self):
        """ssv_rt_finish -> _abi.RtResult: host memory of the context, valid until the next rt_begin (decode it with rt_decode)"""
        r = _abi.RtResult()
        self._check(self._lib.ssv_rt_finish(self._h, C.byref(r)), "ssv_rt_finish")
        return r

    @staticmethod
    def rt_decode(r, target_names=()):
        """the pairs of an _abi.RtResult as dicts (see readthrough)"""
        nt = len(target_names)
        ctg = (lambda t: target_names[t]) if nt else (lambda t: t)
        out = []
        for k in range(r.n_pairs):
            q = r.pairs[k]
            seqs = C.string_at(r.seqs + q.seq_off, q.up_len + q.down_len).decode() if q.up_len + q.down_len else ""
            ops = [r.cigars[q.cig_off + j] for j in range(q.up_cig_n + q.down_cig_n)]
            out.append(dict(key=(ctg(q.up_tid), q.up_pos, chr(q.up_strand), ctg(q.down_tid), q.down_pos, chr(q.down_strand)),
                            microhomology=q.microhomology, kind=q.kind, up_seq=seqs[:q.up_len], down_seq=seqs[q.up_len:],
                            clipped=(q.up_left_clipped, q.up_right_clipped, q.down_left_clipped, q.down_right_clipped),
                            up_cigar=ops[:q.up_cig_n], down_cigar=ops[q.up_cig_n:], edits=(q.up_cig_edit, q.down_cig_edit),
                            records=(q.first_record, q.second_record)))
        return out

    # ---- device-side BGZF inflate + BAM decode ----
    def bamdec_target_lens(self, lens):
        """after ssv_bamdec_begin: the contig lengths sharpen the speculation of record starts (results do not depend on it)"""
        arr = (C.c_int32 * max(1, len(lens)))(*[int(x) for x in lens])
        self._check(self._lib.ssv_bamdec_target_lens(self._h, arr), "ssv_bamdec_target_lens")

    @staticmethod
    def _info_dict(info, hl):
        """an ssv_bamdec_info (ssv_bamdec_last, ssv_samdec_lists) as a dict: the contig changes as (record, contig) pairs, the side channel's records as they
        lie there (unmapped_raw) and as ssvh_raw_record_fastq reads them (unmapped: name, bases, qualities, first of pair)"""
        d = dict(n_records=info.n_records, inflated_bytes=info.inflated_bytes, repaired_blocks=info.repaired_blocks, last_tid=info.last_tid)
        k = info.n_tid_runs
        d["tid_runs"] = list(zip(np.ctypeslib.as_array((C.c_uint32 * k).from_address(info.tid_run_index)).tolist(), np.ctypeslib.as_array((C.c_int32 * k).from_address(info.tid_run_tid)).tolist())) if k else []
        d["unmapped_raw"] = C.string_at(info.unmapped_raw, info.unmapped_bytes) if info.unmapped_bytes else b""
        unm, off = [], 0
        q, sq, ql, r1 = C.c_char_p(), C.c_char_p(), C.c_char_p(), C.c_int()
        while info.unmapped_bytes:
            nxt = hl.ssvh_raw_record_fastq(info.unmapped_raw, info.unmapped_bytes, off, C.byref(q), C.byref(sq), C.byref(ql), C.byref(r1))
            if nxt == 0:
                break
            unm.append((q.value.decode(), sq.value.decode(), ql.value.decode(), bool(r1.value)))
            off = nxt
        d["unmapped"] = unm
        return d

    def bamdec_names(self):
        """ssv_bamdec_names: where the read names of the batch bam_batches handed out last lie in HBM (valid as long as that batch)"""
        n = _abi.Names()
        self._check(self._lib.ssv_bamdec_names(self._h, C.byref(n)), "ssv_bamdec_names")
        return n

    def bam_batches(self, reader, chunk_bytes=64 << 20, max_blocks=1 << 16, keep_all_seq=False, chunk_inflated=1 << 31, prefetch=True, verify_crc=False, any_order=False):
        """Generator over SSV_MEM_DEVICE batches of a whole BAM file (host.BamReader), decoded on the GPU: yields (Batch, info dict).
        The batch is valid until the next iteration.  prefetch: chunk k+1 is read into the second staging buffer and announced
        (ssv_bamdec_prefetch) before chunk k is decoded, so its bytes cross PCIe while chunk k's kernels run."""
        hl = reader._lib
        first = C.c_uint64()
        if hl.ssvh_bam_raw_begin(reader.handle, C.byref(first)) != 0:
            raise IOError(hl.ssvh_last_error().decode())
        self._check(self._lib.ssv_bamdec_begin(self._h, len(reader.target_names), first.value), "ssv_bamdec_begin")
        self.bamdec_target_lens(reader.target_lens)
        if any_order:    # a file in read order (getsv -F): any number of contig changes per chunk
            self._check(self._lib.ssv_bamdec_any_order(self._h, 1), "ssv_bamdec_any_order")
        if verify_crc:   # every inflated block against the CRC32 in its BGZF trailer (off by default, like libbam 0.1.16)
            self._check(self._lib.ssv_bamdec_verify_crc(self._h, 1), "ssv_bamdec_verify_crc")
        stages, blocks = [None, None], [None, None]

        def read(k):
            """chunk k into staging buffer k & 1; its compressed bytes leave for the GPU at once (ssv_bamdec_prefetch)"""
            w = k & 1
            if stages[w] is None:
                stages[w] = C.c_void_p()
                self._check(self._lib.ssv_bamdec_staging(self._h, w, chunk_bytes, C.byref(stages[w])), "ssv_bamdec_staging")
                blocks[w] = (_abi.BgzfBlock * max_blocks)()
            nb, nbytes = C.c_int64(), C.c_size_t()
            if hl.ssvh_bam_read_blocks(reader.handle, stages[w], chunk_bytes, chunk_inflated, blocks[w], max_blocks, C.byref(nb), C.byref(nbytes)) != 0:
                raise IOError(hl.ssvh_last_error().decode())
            if nb.value and prefetch:
                self._check(self._lib.ssv_bamdec_prefetch(self._h, stages[w], nbytes.value), "ssv_bamdec_prefetch")
            return nb, nbytes

        ci, cur = 0, read(0)
        while True:
            nb, nbytes = cur
            if nb.value:
                cur = read(ci + 1)  # read (and announced) before this chunk's kernels start: its upload runs beside them
            b = _abi.Batch()
            self._check(self._lib.ssv_bamdec_decode(self._h, stages[ci & 1], nbytes.value, blocks[ci & 1], nb.value, int(keep_all_seq), C.byref(b)), "ssv_bamdec_decode")
            ci += 1
            if nb.value == 0:
                return
            info = _abi.BamdecInfo()
            self._check(self._lib.ssv_bamdec_last(self._h, C.byref(info)), "ssv_bamdec_last")
            d = self._info_dict(info, hl)
            d.update(n_blocks=nb.value, compressed_bytes=nbytes.value)
            yield b, d

    # ---- device-side SAM text decode (getsv -F on `bwa bwasw` output) ----
    def samdec_begin(self, target_names, first_line=1):
        """ssv_samdec_begin: a new SAM text file whose header names these contigs; first_line: the file's line number of the first record line"""
        arr = (C.c_char_p * max(1, len(target_names)))(*[x.encode() if isinstance(x, str) else x for x in target_names])
        p = _abi.SamdecParams(len(target_names), 0, arr, int(first_line))
        self._check(self._lib.ssv_samdec_begin(self._h, C.byref(p)), "ssv_samdec_begin")

    def samdec_decode(self, text, last=False):
        """ssv_samdec_decode: the next bytes of the file (bytes, cut anywhere) -> Batch (SSV_MEM_DEVICE, valid until the next decode)"""
        b = _abi.Batch()
        buf = C.create_string_buffer(text, len(text)) if len(text) else None
        self._check(self._lib.ssv_samdec_decode(self._h, buf, len(text), _abi.MEM_HOST, int(bool(last)), C.byref(b)), "ssv_samdec_decode")
        return b

    def samdec_sorted(self, keep_all_seq=False):
        """ssv_samdec_sorted, between samdec_begin and the first samdec_decode: the text is a coordinate-sorted original - batches as bam_batches gives them for
        the BAM of the same records, and samdec_lists() behind every decode"""
        self._check(self._lib.ssv_samdec_sorted(self._h, int(bool(keep_all_seq))), "ssv_samdec_sorted")

    def samdec_lists(self):
        """ssv_samdec_lists: the contig changes and the UNMAP|MUNMAP records of the chunk decoded last, as bam_batches' info dict has them"""
        info = _abi.BamdecInfo()
        self._check(self._lib.ssv_samdec_lists(self._h, C.byref(info)), "ssv_samdec_lists")
        return self._info_dict(info, _abi.host_lib())

    def samdec_names(self):
        """ssv_samdec_names: where the read names of the batch decoded last lie in HBM (valid as long as that batch)"""
        n = _abi.Names()
        self._check(self._lib.ssv_samdec_names(self._h, C.byref(n)), "ssv_samdec_names")
        return n

    def samdec_last(self):
        info = _abi.SamdecInfo()
        self._check(self._lib.ssv_samdec_last(self._h, C.byref(info)), "ssv_samdec_last")
        return dict(n_records=info.n_records, lines_consumed=info.lines_consumed, carried_bytes=info.carried_bytes, refused_line=info.refused_line,
                    refused_reason=info.refused_reason.decode() if info.refused_reason else None)

    def sam_batches(self, text, target_names, first_line=1, chunk_bytes=64 << 20, cuts=None):
        """Generator over the SSV_MEM_DEVICE batches of SAM record text (bytes, the file behind its header) decoded on the GPU: yields (Batch, Names).
        The text is handed over in chunks of chunk_bytes, or cut at the byte offsets `cuts`; both are valid until the next iteration."""
        self.samdec_begin(target_names, first_line)
        bounds = sorted(set(cuts)) if cuts is not None else list(range(chunk_bytes, len(text), chunk_bytes))
        bounds = [0] + [x for x in bounds if 0 < x < len(text)] + [len(text)]
        for k in range(len(bounds) - 1):
            b = self.samdec_decode(text[bounds[k]:bounds[k + 1]], last=k == len(bounds) - 2)
            yield b, self.samdec_names()

    # ---- getsv: the clipped-sequence re-alignments as the host join reads them (ssv_aln_pack) ----
    def aln_pack(self, batch, names):
        """ssv_aln_pack: a batch (dict of host arrays, or an _abi.Batch - a decoder's device batch) and its read names (list of str / bytes, or an _abi.Names:
        samdec_names() / bamdec_names()) -> dict of numpy copies of the join's columns (tid, pos, flag, n_cigar, mapq, cigar_off, cigar, name_off, name_hash,
        names_blob: the names back to back with their NULs, name_bytes) plus `names`, the list of names (bytes)"""
        bb, keep = self._as_batch(batch)
        n, keep_names = self._as_names(names)
        c = _abi.AlnCols()
        self._check(self._lib.ssv_aln_pack(self._h, C.byref(bb), C.byref(n), C.byref(c)), "ssv_aln_pack")

        def col(ptr, dt, cnt):
            if not cnt:
                return np.zeros(0, dtype=dt)
            return np.frombuffer((C.c_uint8 * (cnt * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt, count=cnt).copy()

        out = dict(n=int(c.n), name_bytes=int(c.name_bytes), tid=col(c.tid, np.int32, c.n), pos=col(c.pos, np.int32, c.n), flag=col(c.flag, np.uint16, c.n),
                   n_cigar=col(c.n_cigar, np.uint16, c.n), mapq=col(c.mapq, np.uint8, c.n), cigar_off=col(c.cigar_off, np.uint32, c.n),
                   cigar=col(c.cigar, np.uint32, c.n_cigar_total), name_off=col(c.name_off, np.uint64, c.n), name_hash=col(c.name_hash, np.uint64, c.n))
        blob = col(c.names, np.uint8, c.name_bytes).tobytes()
        out["names_blob"] = blob
        out["names"] = [blob[int(a):blob.index(b"\0", int(a))] for a in out["name_off"]]
        return out

    def batch_retain(self, dev_batch):
        """a device batch (the decoder's: valid until the next decode) copied into device memory of its own; -> Batch (SSV_MEM_DEVICE |
        SSV_MEM_PERSISTENT), to be given back with batch_release"""
        out = _abi.Batch()
        self._check(self._lib.ssv_batch_retain(self._h, C.byref(dev_batch), C.byref(out)), "ssv_batch_retain")
        return out

    def batch_release(self, batch):
        self._check(self._lib.ssv_batch_release(self._h, C.byref(batch)), "ssv_batch_release")

    # ---- duplicate read pairs marked while the sample is retained (ssv_dup_*: `seeksv run -M`) ----
    def dup_begin(self):
        """ssv_dup_begin: a new stream of batches in file order"""
        self._check(self._lib.ssv_dup_begin(self._h), "ssv_dup_begin")

    def dup_retain(self, batch, names, last=False):
        """ssv_dup_retain in the place of batch_retain: the decoder's device batch (with every record's qualities) and its names (bamdec_names() /
        samdec_names(), or a list) -> (Batch, carried): a retained batch with final flags - the `carried` records held back by the call before, then
        this batch's records up to its own trailing run (all of them with last) - to be given back with batch_release"""
        n, keep_names = self._as_names(names)
        out, carried = _abi.Batch(), C.c_int64()
        self._check(self._lib.ssv_dup_retain(self._h, C.byref(batch), C.byref(n), int(bool(last)), C.byref(out), C.byref(carried)), "ssv_dup_retain")
        return out, carried.value

    def dup_finish(self):
        """ssv_dup_finish -> dict of the stream's counts (ssv_dup_stats)"""
        st = _abi.DupStats()
        self._check(self._lib.ssv_dup_finish(self._h, C.byref(st)), "ssv_dup_finish")
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    # ---- an original in any order, coordinate sorted while it is retained (ssv_batch_sort: `seeksv run -u`) ----
    def batch_sort(self, batches, n_targets, max_out_records=0):
        """ssv_batch_sort: retained batches (batch_retain's) in input order -> dict(n_records, already_sorted, batches: the retained batches that hold the
        records stably sorted by the rule of include/seeksv_hip.h, each to be given back with batch_release, changes: per output batch the (record, contig)
        pairs where the contig changes among the records without UNMAP|MUNMAP).  On success the inputs are the call's (released, or - already sorted -
        handed back as the outputs); on failure they are still the caller's."""
        arr = (_abi.Batch * max(1, len(batches)))(*batches)
        out = _abi.Sorted()
        self._check(self._lib.ssv_batch_sort(self._h, arr, len(batches), int(n_targets), int(max_out_records), C.byref(out)), "ssv_batch_sort")
        res, changes = [], []
        for k in range(out.n_batches):
            b = _abi.Batch()
            C.memmove(C.byref(b), C.byref(out.batches[k]), C.sizeof(_abi.Batch))
            res.append(b)
            lo, hi = out.change_first[k], out.change_first[k + 1]
            changes.append([(int(out.change_index[j]), int(out.change_tid[j])) for j in range(lo, hi)])
        return dict(n_records=int(out.n_records), already_sorted=bool(out.already_sorted), batches=res, changes=changes)

    # ---- duplicate read pairs by the unclipped 5' ends of both reads, in any record order (ssv_pairdup_*: `seeksv run -D`) ----
    def pairdup_retain(self, batch, names):
        """ssv_pairdup_retain in the place of batch_retain: the decoder's device batch (with every record's qualities) and its names (bamdec_names() /
        samdec_names(), or a list) -> Batch: a retained batch in dup_retain's form that carries one row per record for pairdup_mark, to be given back
        with batch_release"""
        n, keep_names = self._as_names(names)
        out = _abi.Batch()
        self._check(self._lib.ssv_pairdup_retain(self._h, C.byref(batch), C.byref(n), C.byref(out)), "ssv_pairdup_retain")
        return out

    def pairdup_rows(self, batch):
        """the rows of a batch of pairdup_retain that no pairdup_mark has used yet -> numpy array of _abi.PAIRDUP_ROW_DTYPE (tests)"""
        dev = C.c_void_p()
        self._check(self._lib.ssv_pairdup_rows(self._h, C.byref(batch), C.byref(dev)), "ssv_pairdup_rows")
        rows = np.zeros(int(batch.n), dtype=_abi.PAIRDUP_ROW_DTYPE)
        self._check(self._lib.ssv_pairdup_rows_to_host(self._h, C.byref(batch), rows.ctypes.data if len(rows) else None), "ssv_pairdup_rows_to_host")
        return rows

    def pairdup_mark(self, batches):
        """ssv_pairdup_mark: the rule's 0x400 into the record lines of all the batches of pairdup_retain (one sequence in this order), in place -> dict of
        the counts (ssv_pairdup_stats).  The batches stay the caller's: ordinary retained batches afterwards."""
        arr = (_abi.Batch * max(1, len(batches)))(*batches)
        st = _abi.PairdupStats()
        self._check(self._lib.ssv_pairdup_mark(self._h, arr, len(batches), C.byref(st)), "ssv_pairdup_mark")
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    # ---- the retained records restricted to a list of regions (ssv_regions_set, ssv_region_retain, ssv_batch_select: `seeksv run -L`, `-X`) ----
    def regions_set(self, regions, n_targets, exclude=False):
        """ssv_regions_set: the list of (tid, s, t) triples, normalised as include/seeksv_hip.h says (sorted, merged, clipped), for the calls below;
        exclude: a record is kept iff it overlaps none of them"""
        arr = (_abi.Region * max(1, len(regions)))(*[_abi.Region(int(t), int(s), int(e)) for t, s, e in regions])
        self._check(self._lib.ssv_regions_set(self._h, arr, len(regions), int(n_targets), int(bool(exclude))), "ssv_regions_set")

    def regions_clear(self):
        self._check(self._lib.ssv_regions_clear(self._h), "ssv_regions_clear")

    def region_lds_capacity(self):
        """how many regions of one contig the selection stages in LDS; a longer list is searched in global memory"""
        return int(self._lib.ssv_region_lds_capacity())

    @staticmethod
    def _region_info(info):
        return dict(n_in=int(info.n_in), n_kept=int(info.n_kept), uncopied=bool(info.uncopied), last_tid=int(info.last_tid),
                    changes=[(int(info.change_index[j]), int(info.change_tid[j])) for j in range(info.n_changes)])

    def region_retain(self, dev_batch, last_tid=0):
        """ssv_region_retain in the place of batch_retain: the decoder's device batch -> (Batch, info): a retained batch of the records the list keeps, to be
        given back with batch_release, and dict(n_in, n_kept, uncopied, last_tid: what to pass with the next batch, changes: the (record, contig) pairs
        where the contig changes among the output's records without UNMAP|MUNMAP)"""
        out, info = _abi.Batch(), _abi.RegionInfo()
        self._check(self._lib.ssv_region_retain(self._h, C.byref(dev_batch), int(last_tid), C.byref(out), C.byref(info)), "ssv_region_retain")
        return out, self._region_info(info)

    def batch_select(self, batch, last_tid=0):
        """ssv_batch_select: a retained batch -> (Batch, info) as region_retain.  On success the input is the call's (released, or - every record kept -
        handed back as the output: info["uncopied"]) and zeroed; on failure it is still the caller's."""
        out, info = _abi.Batch(), _abi.RegionInfo()
        self._check(self._lib.ssv_batch_select(self._h, C.byref(batch), int(last_tid), C.byref(out), C.byref(info)), "ssv_batch_select")
        return out, self._region_info(info)

    def samdec_any_order(self, on=True):
        """ssv_samdec_any_order, after samdec_begin: text in any record order - a chunk with more contig changes than the list holds is decoded all the same,
        without its contig-change list"""
        self._check(self._lib.ssv_samdec_any_order(self._h, int(bool(on))), "ssv_samdec_any_order")

    def batch_lines(self, dev_batch):
        """the record lines of a device batch (a retained one too) -> numpy array of _abi.RECORD_DTYPE (a hook of the tests, no part of the C ABI)"""
        lines = np.zeros(int(dev_batch.n), dtype=_abi.RECORD_DTYPE)
        self._check(self._lib.ssv_batch_lines_to_host(self._h, C.byref(dev_batch), lines.ctypes.data if len(lines) else None), "ssv_batch_lines_to_host")
        return lines

    def batch_to_host(self, dev_batch):
        """Device batch -> dict of owned numpy arrays (tests)."""
        h = _abi.Batch()
        self._check(self._lib.ssv_batch_to_host(self._h, C.byref(dev_batch), C.byref(h)), "ssv_batch_to_host")
        return _abi.batch_to_arrays(h)

    # ---- getclip ----
    def clip_begin(self, match_rate=0.9, min_mapq=1, save_low_quality=False, own=None, initial_last_tid=0):
        p = _abi.ClipParams.make(match_rate, min_mapq, save_low_quality, own, initial_last_tid)
        self._check(self._lib.ssv_clip_begin(self._h, C.byref(p)), "ssv_clip_begin")

    def clip_table_format(self, packed):
        """0 / False: ASCII; 3: the compact table (2-bit bases, qualities as alphabet indices, contig / side as runs: a third of the bytes over
        PCIe); host.cluster_strings decodes both"""
        self._check(self._lib.ssv_clip_table_format(self._h, int(packed)), "ssv_clip_table_format")

    def clip_scan(self, batch):
        b, keep = self._as_batch(batch)
        self._check(self._lib.ssv_clip_scan(self._h, C.byref(b)), "ssv_clip_scan")

    def clip_event_count(self):
        n = C.c_int64()
        self._check(self._lib.ssv_clip_event_count(self._h, C.byref(n)), "ssv_clip_event_count")
        return n.value

    def clip_cluster(self, as_dict=True):
        t = _abi.HipClusterTable()
        self._check(self._lib.ssv_clip_cluster(self._h, C.byref(t)), "ssv_clip_cluster")
        return table_to_dict(t) if as_dict else t

    def clip_cluster_async(self):
        """Cluster and queue the table's copy to the host; -> (n_clusters, n_events).  Collect with clip_table_wait()."""
        nc, ne = C.c_int64(), C.c_int64()
        self._check(self._lib.ssv_clip_cluster_async(self._h, C.byref(nc), C.byref(ne)), "ssv_clip_cluster_async")
        return nc.value, ne.value

    def clip_table_wait(self, prev=False, as_dict=False):
        t = _abi.HipClusterTable()
        fn = self._lib.ssv_clip_table_wait_prev if prev else self._lib.ssv_clip_table_wait
        self._check(fn(self._h, C.byref(t)), "ssv_clip_table_wait")
        return table_to_dict(t) if as_dict else t

    def clip_table_expand(self, t, n_threads=0):
        """format 3: rebuild the columns that did not cross PCIe (ssv_clip_table_expand) - sets t's pointers"""
        self._check(self._lib.ssv_clip_table_expand(self._h, C.byref(t), int(n_threads)), "ssv_clip_table_expand")
        return t

    def clip_table_wire_bytes(self, t):
        """what really crossed PCIe for the handed-out table t (ssv_clip_table_wire_bytes) -> dict: narrow, total and the pieces"""
        w = _abi.TableWire()
        self._check(self._lib.ssv_clip_table_wire_bytes(self._h, C.byref(t), C.byref(w)), "ssv_clip_table_wire_bytes")
        return {k: int(getattr(w, k)) for k, _ in _abi.TableWire._fields_ if k != "pad"}

    def clip_scan_range(self, batch, rec_begin, rec_end):
        b, keep = self._as_batch(batch)
        self._check(self._lib.ssv_clip_scan_range(self._h, C.byref(b), int(rec_begin), int(rec_end)), "ssv_clip_scan_range")

    def getclip(self, batches, match_rate=0.9, min_mapq=1, save_low_quality=False, own=None, initial_last_tid=0, tid_runs=None):
        """InputBamOutputReads' record loop over a list of batches -> cluster table dict.
        Contigs that come back (unsorted input): the reference flushes its maps at every change of contig among the mapped-pair records
        (clip_reads.h:423-438); a pass of the library bins by (contig, side, position), so the pass ends in front of a visit whose contig is
        not greater than every contig the pass has seen, and the tables of the passes follow each other (see ssv_clip_scan_range).
        tid_runs: per batch the list of (record index, contig) changes - computed here for batches given as arrays; a device batch without
        it is taken as coordinate sorted."""
        tables = []
        self.clip_begin(match_rate, min_mapq, save_low_quality, own, initial_last_tid)
        last_tid = pass_max = int(initial_last_tid)
        for bi, b in enumerate(batches):
            runs = tid_runs[bi] if tid_runs is not None else (host_tid_runs(b, last_tid) if isinstance(b, dict) and b.get("flag") is not None else [])
            n = len(b["tid"]) if isinstance(b, dict) else int(b.n)
            lo = 0
            for i, tid in runs:
                if tid <= pass_max and own is None:
                    self.clip_scan_range(b, lo, i)
                    tables.append(self.clip_cluster())
                    self.clip_begin(match_rate, min_mapq, save_low_quality, own, last_tid)
                    lo, pass_max = i, tid
                pass_max = max(pass_max, tid)
                last_tid = tid
            self.clip_scan_range(b, lo, n)
        tables.append(self.clip_cluster())
        return tables[0] if len(tables) == 1 else concat_tables(tables)

    # ---- somatic: look-ups among a pass's clusters where they lie ----
    def clip_probe_set(self, probes, match_rate=0.9, min_clipped_len=10):
        """probes: dicts (tid, lo, hi, side, mode, a, b) or tuples in that order; side '3' / '5' (or its code), a / b str or bytes.  They stay set - every
        clip_cluster runs them against its table (format 0) - until a set with no probes, the next set, or the context's end (ssv_clip_probe_set)."""
        keys = ("tid", "lo", "hi", "side", "mode", "a", "b")
        arr = np.zeros(len(probes), dtype=_abi.CLIP_PROBE_DTYPE)
        text = bytearray()
        for i, p in enumerate(probes):
            tid, lo, hi, side, mode, a, b = (p[k] for k in keys) if isinstance(p, dict) else p
            a, b = (x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in (a, b))
            side = ord(side) if isinstance(side, (str, bytes)) else int(side)
            arr[i] = (tid, lo, hi, side, mode, (0, 0), len(text), len(a), len(text) + len(a), len(b))
            text += a + b
        buf = (C.c_char * max(len(text), 1)).from_buffer_copy(bytes(text) or b"\0")
        self._check(self._lib.ssv_clip_probe_set(self._h, arr.ctypes.data if len(arr) else None, len(arr), C.addressof(buf), len(text), float(match_rate), int(min_clipped_len) & 0xffffffff),
                    "ssv_clip_probe_set")
        self._n_probes = len(arr)

    def clip_probe_get(self):
        """-> (hits: structured array support / pos / pass / cluster per probe, support 0 = no cluster matched; passes clustered since the set)"""
        hits = np.zeros(getattr(self, "_n_probes", 0), dtype=_abi.CLIP_PROBE_HIT_DTYPE)
        passes = C.c_int64()
        self._check(self._lib.ssv_clip_probe_get(self._h, hits.ctypes.data if len(hits) else None, C.byref(passes)), "ssv_clip_probe_get")
        return hits, passes.value

    # ---- getsv pass 1 ----
    def isize_stats(self, batches, min_mapq=20, max_pairs=5000000):
        """-> (rc, n_pairs, mean, sd); rc == 1 when no pair qualifies (the reference's return value)."""
        self._check(self._lib.ssv_isize_begin(self._h, min_mapq, max_pairs), "ssv_isize_begin")
        done = C.c_int32(0)
        for bt in batches:
            b, keep = self._as_batch(bt)
            self._check(self._lib.ssv_isize_accumulate(self._h, C.byref(b), C.byref(done)), "ssv_isize_accumulate")
            if done.value:
                break
        n, mean, sd = C.c_int64(), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.ssv_isize_finish(self._h, C.byref(n), C.byref(mean), C.byref(sd)), "ssv_isize_finish")
        return (1 if n.value == 0 else 0), n.value, mean.value, sd.value

    # ---- getsv passes 2+3 ----
    def getsv_begin(self, junctions, windows, mean, sd, target_lens, times=4, disc_min_mapq=20, depth_min_mapq=20):
        j = np.ascontiguousarray(junctions, dtype=_abi.JUNCTION_DTYPE)
        w = np.ascontiguousarray(windows, dtype=_abi.INTERVAL_DTYPE)
        tl = np.ascontiguousarray(target_lens, dtype=np.int32)
        p = _abi.GetsvParams()
        p.junctions = j.ctypes.data if len(j) else None
        p.n_junctions = len(j)
        p.mean, p.sd, p.times, p.disc_min_mapq = mean, sd, times, disc_min_mapq
        p.windows = w.ctypes.data if len(w) else None
        p.n_windows = len(w)
        p.depth_min_mapq = depth_min_mapq
        p.n_targets = len(tl)
        p.target_len = tl.ctypes.data if len(tl) else None
        self._gs_nj = len(j)
        self._check(self._lib.ssv_getsv_begin(self._h, C.byref(p)), "ssv_getsv_begin")

    def getsv_scan(self, batch):
        b, keep = self._as_batch(batch)
        self._check(self._lib.ssv_getsv_scan(self._h, C.byref(b)), "ssv_getsv_scan")

    def getsv_finish(self, ranges, points):
        r = np.ascontiguousarray(ranges, dtype=_abi.INTERVAL_DTYPE)
        q = np.ascontiguousarray(points, dtype=_abi.INTERVAL_DTYPE)
        counts = np.zeros(self._gs_nj, dtype=np.int32)
        rs = np.zeros(len(r), dtype=np.uint64)
        pd = np.zeros(len(q), dtype=np.int32)
        mx = C.c_int32(0)
        ptr = lambda a: a.ctypes.data if a.size else None
        self._check(self._lib.ssv_getsv_finish(self._h, ptr(counts), ptr(r), len(r), ptr(rs), ptr(q), len(q), ptr(pd), C.byref(mx)), "ssv_getsv_finish")
        return counts, rs, pd, mx.value

    def discordant_and_depth(self, batches, plan, mean, sd, min_mapq, target_lens):
        """Backend protocol shared with the oracle in the tests (see tests/golden_util.py)."""
        self.getsv_begin(plan.junctions, plan.windows, mean, sd, target_lens, 4, min_mapq, min_mapq)
        for b in batches:
            self.getsv_scan(b)
        counts, rs, pd, _ = self.getsv_finish(plan.ranges, plan.points)
        return counts, rs, pd

    # ---- clipped-sequence re-aligner (stand-in for the pipeline's external `bwa mem` step) ----
    def realign_index(self, ref2bit, target_off, mem=_abi.MEM_HOST):
        """ref2bit: numpy uint64 array (host) or a device pointer (mem=MEM_DEVICE); target_off: first base of every contig + total"""
        off = np.ascontiguousarray(target_off, np.int64)
        ptr = ref2bit.ctypes.data if isinstance(ref2bit, np.ndarray) else int(ref2bit)
        dropped = C.c_int64()
        self._check(self._lib.ssv_realign_index(self._h, ptr, mem, int(off[-1]), off.ctypes.data, len(off) - 1, C.byref(dropped)), "ssv_realign_index")
        return dropped.value

    def realign_index_sorted(self, ref2bit, target_off, max_occ, mem=_abi.MEM_HOST):
        """the sorted index (references with repeats): query 20-mers with more than max_occ occurrences give no seed.  Arguments as realign_index;
        -> dict(n_indexed, n_distinct, occ_max, n_over_cap).  realign() then uses this index; its flags are hits["pad"][:, 0] (_abi.RA_F_*)."""
        off = np.ascontiguousarray(target_off, np.int64)
        ptr = ref2bit.ctypes.data if isinstance(ref2bit, np.ndarray) else int(ref2bit)
        st = _abi.RealignIndexStats()
        self._check(self._lib.ssv_realign_index_sorted(self._h, ptr, mem, int(off[-1]), off.ctypes.data, len(off) - 1, int(max_occ), C.byref(st)), "ssv_realign_index_sorted")
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    @staticmethod
    def _realign_io(seqs):
        """list of str -> (the sequences back to back, their offsets [n + 1], zeroed ssv_realign_hit [n])"""
        off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.uint64)
        return "".join(seqs).encode(), off, np.zeros(len(seqs), dtype=np.dtype(_abi.REALIGN_HIT))

    def realign(self, seqs, gapped=False):
        """list of str -> numpy structured array of ssv_realign_hit; gapped: one insertion or deletion per alignment (ssv_realign_query_gapped)
        -> (hits, structured array of ssv_realign_gap)"""
        blob, off, hits = self._realign_io(seqs)
        if not gapped:
            if len(seqs):
                self._check(self._lib.ssv_realign_query(self._h, C.c_char_p(blob), off.ctypes.data, len(seqs), hits.ctypes.data), "ssv_realign_query")
            return hits
        gaps = np.zeros(len(seqs), dtype=np.dtype(_abi.REALIGN_GAP))
        if len(seqs):
            self._check(self._lib.ssv_realign_query_gapped(self._h, C.c_char_p(blob), off.ctypes.data, len(seqs), hits.ctypes.data, gaps.ctypes.data), "ssv_realign_query_gapped")
        return hits, gaps

    def realign_alts(self, seqs, max_alt, gapped=False):
        """realign() + every query's other loci (ssv_realign_query_alts, max_alt in 1..16) -> (hits, gaps or None, alt_off, alts): query i's alternates
        are alts[alt_off[i]:alt_off[i + 1]], in the rule's order; hits["pad"][:, 0] & _abi.RA_F_ALT_CUT where more loci qualified than max_alt"""
        n = len(seqs)
        blob, off, hits = self._realign_io(seqs)
        gaps = np.zeros(n, dtype=np.dtype(_abi.REALIGN_GAP)) if gapped else None
        alt_off = np.full(n + 1, -1, dtype=np.int64)
        alts = np.zeros(max(n * max(int(max_alt), 0), 1), dtype=np.dtype(_abi.REALIGN_HIT))
        self._check(self._lib.ssv_realign_query_alts(self._h, C.c_char_p(blob), off.ctypes.data, n, int(max_alt), 1 if gapped else 0, hits.ctypes.data,
                                                     gaps.ctypes.data if gapped else None, alt_off.ctypes.data, alts.ctypes.data), "ssv_realign_query_alts")
        return hits, gaps, alt_off, alts[:int(alt_off[n])].copy()

    def realign_split(self, seqs):
        """realign() for whole reads that may cross a breakpoint (ssv_realign_query_split) -> (hits, mates): mates[i] is read i's second piece, or
        unaligned (tid -1, the primary's flags in pad[0]); with a mate, hits[i]'s second / mapq count only competitors for the primary's own part"""
        n = len(seqs)
        blob, off, hits = self._realign_io(seqs)
        mates = np.zeros(max(n, 1), dtype=np.dtype(_abi.REALIGN_HIT))
        self._check(self._lib.ssv_realign_query_split(self._h, C.c_char_p(blob), off.ctypes.data, n, hits.ctypes.data, mates.ctypes.data), "ssv_realign_query_split")
        return hits, mates[:n]

    def realign_split_batch(self, seqs, names, quals=None):
        """realign_split() + the records `seeksv realign -P` writes, built on the GPU (ssv_realign_split_batch).  seqs, names (and quals: phred + 33, as
        long as their reads): lists of str -> (hits, mates, Batch, Names); the batch and its names are SSV_MEM_DEVICE, owned by the context and valid until
        its next realign call: rt_scan() takes them in place, batch_to_host() / aln_pack() copy them out.  A read with a mate gives two records."""
        n = len(seqs)
        if len(names) != n or (quals is not None and [len(x) for x in quals] != [len(x) for x in seqs]):
            raise ValueError("realign_split_batch: one name per read, qualities as long as their reads")
        blob, off, hits = self._realign_io(seqs)
        mates = np.zeros(max(n, 1), dtype=np.dtype(_abi.REALIGN_HIT))
        hits = hits if n else np.zeros(1, dtype=np.dtype(_abi.REALIGN_HIT))
        raw = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
        nblob = b"".join(x + b"\0" for x in raw)
        noff = np.concatenate([[0], np.cumsum([len(x) + 1 for x in raw])]).astype(np.uint64)
        qblob = C.c_char_p("".join(quals).encode()) if quals is not None else None
        b, nm = _abi.Batch(), _abi.Names()
        self._check(self._lib.ssv_realign_split_batch(self._h, C.c_char_p(blob), off.ctypes.data, n, qblob, C.c_char_p(nblob), noff.ctypes.data, hits.ctypes.data,
                                                      mates.ctypes.data, C.byref(b), C.byref(nm)), "ssv_realign_split_batch")
        return hits[:n], mates[:n], b, nm

    # ---- measurement ----
    def prof_enable(self, mode=1):
        self._check(self._lib.ssv_prof_enable(self._h, mode), "ssv_prof_enable")

    def prof_reset(self):
        self._check(self._lib.ssv_prof_reset(self._h), "ssv_prof_reset")

    def prof_get(self, name):
        ms, n, u = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self._lib.ssv_prof_get(self._h, name.encode(), C.byref(ms), C.byref(n), C.byref(u)), "ssv_prof_get")
        return dict(total_ms=ms.value, launches=n.value, units=u.value)

    def prof_all(self):
        return {n: self.prof_get(n) for n in self._lib.ssv_prof_names().decode().split("\n")}


class PinnedArrays:
    """numpy arrays in page-locked host memory (ssv_host_alloc): only out of such memory do the copies of a host batch run asynchronously"""

    def __init__(self):
        self._lib = _abi.hip_lib()
        self._ptrs = []

    def empty(self, n, dtype):
        dt = np.dtype(dtype)
        p = C.c_void_p()
        if self._lib.ssv_host_alloc(max(1, int(n) * dt.itemsize), C.byref(p)) != 0:
            raise SeeksvError("ssv_host_alloc failed")
        self._ptrs.append(p)
        return np.frombuffer((C.c_uint8 * (int(n) * dt.itemsize)).from_address(p.value), dtype=dt, count=int(n))

    def copy(self, a):
        a = np.ascontiguousarray(a)
        out = self.empty(a.size * a.dtype.itemsize, np.uint8).view(a.dtype) if a.dtype.fields else self.empty(a.size, a.dtype)
        out[...] = a.reshape(-1)
        return out

    def batch(self, arrays):
        """a host batch (dict of numpy arrays, as synth.Workload.generate_host gives) copied into page-locked memory"""
        return {k: (self.copy(v) if isinstance(v, np.ndarray) else v) for k, v in arrays.items()}

    def close(self):
        for p in self._ptrs:
            self._lib.ssv_host_free(p)
        self._ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
