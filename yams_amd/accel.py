"""Thin numpy-facing wrapper over the C ABI (one context = one device + one stream).

All compute happens in libyams_mi355x_accel.so on the GPU.  Device memory is addressed by integer
pointers (e.g. `tensor.data_ptr()`); `DeviceArray` is a minimal owner for hosts without torch.
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import (AccelError, CdcConfig, IngestResult, ScanCorpus, ScanDiag, ScanDocs, ScanParams,
                   CDC_RABIN, CDC_STREAMING, SCAN_COSINE, SCAN_L2)

DEFAULT_POLY = 0x3DA3358B4DC173


def cdc_config(mode="streaming", window=48, min_size=16 * 1024, max_size=1024 * 1024,
               polynomial=DEFAULT_POLY, mask=0x1FFF, generic_kernel=False) -> CdcConfig:
    m = CDC_STREAMING if mode in ("streaming", CDC_STREAMING) else CDC_RABIN
    return CdcConfig(window, min_size, max_size, polynomial, mask, m,
                     _lib.CDC_FLAG_GENERIC_KERNEL if generic_kernel else 0)


class DeviceArray:
    """Owns a hipMalloc'd buffer; `.ptr` is the device address."""

    def __init__(self, acc: "Accel", nbytes: int):
        self.acc = acc
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        acc._check(acc.L.yams_accel_malloc(acc.ctx, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr: np.ndarray, offset: int = 0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        self.acc._check(self.acc.L.yams_accel_upload(self.acc.ctx, self.ptr + offset,
                                                     arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype, count: int, offset: int = 0) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            self.acc._check(self.acc.L.yams_accel_download(self.acc.ctx, out.ctypes.data,
                                                           self.ptr + offset, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.acc.L.yams_accel_free(self.acc.ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


@dataclass
class ScanResult:
    scores: np.ndarray   # [nq, k] float32 (cosine similarity / relevance_score)
    rows: np.ndarray     # [nq, k] int64
    counts: np.ndarray   # [nq] uint32
    dist: np.ndarray     # [nq, k] float32
    diag: dict


class DedupSet:
    """Device-resident set of SHA-256 digests (chunk dedup lookup)."""

    def __init__(self, acc: "Accel", expected_entries: int = 0):
        self.acc = acc
        self.h = C.c_void_p()
        acc._check(acc.L.yams_dedup_set_create(acc.ctx, expected_entries, C.byref(self.h)))

    def close(self):
        # yams_dedup_set_destroy uses the set's context: once the Accel is closed there is nothing left to call it
        # on (a set kept alive past the context, e.g. by a traceback, is dropped with the process)
        if self.h and getattr(self.acc, "ctx", None):
            self.acc.L.yams_dedup_set_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = C.c_uint64(0)
        self.acc._check(self.acc.L.yams_dedup_set_size(self.h, C.byref(n)))
        return n.value

    def insert(self, digests: np.ndarray) -> np.ndarray:
        """digests: [n][32] uint8 (host).  Returns is_new[n] (bool)."""
        d = np.ascontiguousarray(digests, np.uint8).reshape(-1, 32)
        out = np.zeros(d.shape[0], np.uint8)
        nn = C.c_uint64(0)
        self.acc._check(self.acc.L.yams_dedup_insert_host(self.h, d.ctypes.data_as(C.c_void_p), d.shape[0],
                                                          out.ctypes.data_as(C.c_void_p), C.byref(nn)))
        assert nn.value == int(out.sum())
        return out.astype(bool)

    def probe(self, digests: np.ndarray) -> np.ndarray:
        d = np.ascontiguousarray(digests, np.uint8).reshape(-1, 32)
        out = np.zeros(d.shape[0], np.uint8)
        self.acc._check(self.acc.L.yams_dedup_probe_host(self.h, d.ctypes.data_as(C.c_void_p), d.shape[0],
                                                         out.ctypes.data_as(C.c_void_p)))
        return out.astype(bool)

    def insert_device(self, digests_ptr: int, n: int, sizes_ptr: int | None, is_new_ptr: int):
        nn, bn, bd = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self.acc._check(self.acc.L.yams_dedup_insert_device(self.h, digests_ptr, n, sizes_ptr, is_new_ptr,
                                                            C.byref(nn), C.byref(bn), C.byref(bd)))
        return nn.value, bn.value, bd.value


def pack_candidates(mask: np.ndarray) -> np.ndarray:
    """bool [q][c] -> the bitset yams_route_dense takes: uint32 [q][ceil(c / 32)], bit c % 32 of word c / 32."""
    m = np.asarray(mask, bool)
    q, c = m.shape
    words = (c + 31) // 32
    padded = np.zeros((q, words * 32), np.uint8)
    padded[:, :c] = m
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little").view("<u4").reshape(q, words))


class RouteIndex:
    """Owns a yams_route_index (the resident table of cluster vectors of one topology snapshot)."""

    def __init__(self, acc: "Accel", vectors, cluster_offsets, has_centroid, position, host_entry: bool = False, misalign: int = 0):
        x = np.ascontiguousarray(vectors, np.float32)
        assert x.ndim == 2
        self.acc, self.h = acc, None
        v, self.dim = x.shape
        off = np.ascontiguousarray(cluster_offsets, np.uint32)
        has = np.ascontiguousarray(has_centroid, np.uint8)
        pos = np.ascontiguousarray(position, np.uint16)
        self.n_clusters, self.n_vectors = len(off) - 1, v
        h = C.c_void_p()
        (norms,) = acc._artifact_call(
            acc.L.yams_route_index_create_device, acc.L.yams_route_index_create_host, host_entry,
            [x if x.size else None, off, has if has.size else None, pos if pos.size else None], [(np.float32, v)],
            lambda i, o: (i[0], v, self.dim, i[1], i[2], i[3], self.n_clusters, C.byref(h), o[0]), misalign)
        self.h, self.norms = h, norms

    def info(self) -> dict:
        inf = _lib.RouteIndexInfo()
        self.acc._check(self.acc.L.yams_route_index_info(self.h, C.byref(inf)))
        return {"n_vectors": inf.n_vectors, "n_clusters": inf.n_clusters, "dim": inf.dim, "bytes": inf.bytes}

    def close(self):
        if self.h and getattr(self.acc, "ctx", None):      # (the index uses its context: see DedupSet.close)
            self.acc.L.yams_route_index_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedScan:
    """yams_scan_sharded_*: one search over a corpus row-sharded across several devices behind the C ABI — one
    process, one RCCL communicator over the shard devices, all-gather + merge per batch, `lanes` batches in
    flight (shards that share a device, the one-GPU tests, exchange their records with device copies).
    `ctx(i)` is an Accel bound to shard i's lane-0 context — upload the shard's rows and build its shadows
    through it.  collective: "auto" | "rccl" (require the communicator, also for one shard) | "peer";
    rccl_library: the collective library to bind instead of librccl.so.1 (the tests' stand-in lets ranks share a
    device); fence=False lifts the exchange fence (measurements); exchange_timeout_ms: the deadline of wait()
    (0 = 30 s; a batch that misses it raises AccelError TIMEOUT and the handle is stuck)."""

    def __init__(self, devices, lanes: int = 0, collective: str = "auto", rccl_library: str | None = None, fence: bool = True,
                 exchange_timeout_ms: int = 0):
        self.L = _lib.load()
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        opt = _lib.ShardedOptions(C.sizeof(_lib.ShardedOptions), lanes,
                                  {"auto": _lib.SHARDED_COLLECTIVE_AUTO, "rccl": _lib.SHARDED_COLLECTIVE_RCCL,
                                   "peer": _lib.SHARDED_COLLECTIVE_PEER}[collective],
                                  _lib.SHARDED_FENCE_AUTO if fence else _lib.SHARDED_FENCE_OFF,
                                  rccl_library.encode() if rccl_library else None, exchange_timeout_ms, 0)
        st = self.L.yams_scan_sharded_create_ex(arr, len(devices), C.byref(opt), C.byref(h))
        if st != 0:
            raise AccelError(st, "yams_scan_sharded_create_ex failed")
        self.h = h
        self.n = len(devices)
        self.devices = list(devices)
        self.lanes = self.L.yams_scan_sharded_lanes(h)
        self._views = [self._borrow(i, 0) for i in range(self.n)]
        self._inflight = {}

    def _borrow(self, shard: int, lane: int) -> "Accel":
        a = Accel.__new__(Accel)
        a.L = self.L; a.ctx = C.c_void_p(self.L.yams_scan_sharded_lane_ctx(self.h, shard, lane)); a.device = self.devices[shard]
        a._borrowed = True
        return a

    def ctx(self, i: int) -> "Accel":
        return self._views[i]

    def lane_ctx(self, shard: int, lane: int) -> "Accel":
        """The context lane `lane` uses on shard `shard` (kernel timings of a pipelined run)."""
        return self._borrow(shard, lane)

    def info(self) -> dict:
        p = C.c_void_p()
        st = self.L.yams_scan_sharded_info_json(self.h, C.byref(p))
        if st != 0:
            raise AccelError(st, "yams_scan_sharded_info_json failed")
        try:
            return json.loads(C.string_at(p).decode())
        finally:
            self.L.yams_accel_free_string(p)

    def close(self):
        if getattr(self, "h", None):
            for a in self._views:
                a.ctx = None
            self.L.yams_scan_sharded_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _error(self, st):
        return AccelError(st, self.L.yams_scan_sharded_last_error(self.h).decode())

    # -- pipelined form ------------------------------------------------------------------------------
    def submit(self, shards, queries: np.ndarray, k: int, threshold: float = 0.0, metric: int = SCAN_COSINE,
               flags: int = 0, rank_of_row_ptr: int | None = None, rank_row_base: int = 0, want_diag: bool = True,
               block: bool = True) -> int:
        """Starts one batch on a free lane and returns the lane; wait(lane) returns its merged result."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        lane = C.c_uint32()
        st = self.L.yams_scan_sharded_lane_acquire(self.h, 1 if block else 0, C.byref(lane))
        if st != 0:
            raise self._error(st)
        prm = ScanParams(k, threshold, metric, flags)
        arr = (ScanCorpus * self.n)(*shards)
        st = self.L.yams_scan_sharded_submit(self.h, lane.value, arr, q.ctypes.data, q.shape[0], C.byref(prm), rank_of_row_ptr,
                                             rank_row_base, _lib.SHARDED_SUBMIT_DIAG if want_diag else 0)
        if st != 0:
            self.L.yams_scan_sharded_lane_release(self.h, lane.value)
            raise self._error(st)
        self._inflight[lane.value] = (q.shape[0], k, arr)       # (the views must outlive the batch)
        return lane.value

    def wait(self, lane: int) -> ScanResult:
        nq, k, _ = self._inflight.pop(lane)
        kk = max(k, 1)
        scores = np.full((nq, kk), -np.inf, np.float32)
        rows = np.full((nq, kk), -1, np.int64)
        counts = np.zeros(nq, np.uint32)
        dist = np.full((nq, kk), np.inf, np.float32)
        diag = ScanDiag()
        st = self.L.yams_scan_sharded_wait(self.h, lane, scores.ctypes.data, rows.ctypes.data, counts.ctypes.data,
                                           dist.ctypes.data, C.byref(diag))
        if st != 0:
            raise self._error(st)
        return ScanResult(scores[:, :k], rows[:, :k], counts, dist[:, :k], diag.as_dict())

    # -- one call ------------------------------------------------------------------------------------
    def topk(self, shards, queries: np.ndarray, k: int, threshold: float = 0.0, metric: int = SCAN_COSINE,
             flags: int = 0, rank_of_row_ptr: int | None = None, rank_row_base: int = 0) -> ScanResult:
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq, kk = q.shape[0], max(k, 1)
        scores = np.full((nq, kk), -np.inf, np.float32)
        rows = np.full((nq, kk), -1, np.int64)
        counts = np.zeros(nq, np.uint32)
        dist = np.full((nq, kk), np.inf, np.float32)
        prm = ScanParams(k, threshold, metric, flags)
        diag = ScanDiag()
        arr = (ScanCorpus * self.n)(*shards)
        st = self.L.yams_scan_sharded_topk_host(self.h, arr, q.ctypes.data, nq, C.byref(prm), rank_of_row_ptr,
                                                rank_row_base, scores.ctypes.data, rows.ctypes.data,
                                                counts.ctypes.data, dist.ctypes.data, C.byref(diag))
        if st != 0:
            raise self._error(st)
        return ScanResult(scores[:, :k], rows[:, :k], counts, dist[:, :k], diag.as_dict())


class SweepGate:
    """Shared by the contexts of one device that search concurrently: their filter sweeps run one after the
    other on the GPU, everything around them overlaps (yams_accel_gate_create in the header)."""

    def __init__(self, device: int = 0):
        self.L = _lib.load()
        h = C.c_void_p()
        st = self.L.yams_accel_gate_create(device, C.byref(h))
        if st != 0:
            raise AccelError(st, "yams_accel_gate_create failed")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.yams_accel_gate_destroy(self.h)
        self.h = None


class Accel:
    def __init__(self, device: int = 0, stream: int | None = None):
        """stream: a hipStream_t handle, or None / 0 for a non-blocking stream of the context's own.  torch's DEFAULT stream has
        the handle 0: a context created with torch.cuda.current_stream().cuda_stream while no torch.cuda.Stream is current runs
        on its own stream, unordered with torch's work — torch.cuda.synchronize() before handing it tensors torch has just written."""
        self.L = _lib.load()
        if self.L.yams_accel_device_count() <= 0:
            raise AccelError(_lib.YAMS_ERR_UNSUPPORTED,
                             "no HIP device visible (the accelerator path has no CPU fallback)")
        ctx = C.c_void_p()
        st = self.L.yams_accel_ctx_create(device, C.c_void_p(stream) if stream else None,
                                          C.byref(ctx))
        if st != 0:
            raise AccelError(st, "yams_accel_ctx_create failed")
        self.ctx = ctx
        self.device = device

    def close(self):
        if getattr(self, "ctx", None) and not getattr(self, "_borrowed", False):
            self.L.yams_accel_ctx_destroy(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int):
        if st != 0:
            raise AccelError(st, self.L.yams_accel_last_error(self.ctx).decode())

    def set_sweep_hold(self, on: bool):
        """Keep the sweep gate closed behind this context's sweeps until release_sweep_hold (yams_accel_ctx_set_sweep_hold)."""
        self._check(self.L.yams_accel_ctx_set_sweep_hold(self.ctx, 1 if on else 0))

    def release_sweep_hold(self, stream_ptr: int | None = None):
        self._check(self.L.yams_accel_ctx_release_sweep_hold(self.ctx, C.c_void_p(stream_ptr) if stream_ptr else None))

    def set_gate(self, gate: "SweepGate | None"):
        """Attach this context to a sweep gate (None detaches).  The gate must outlive the context."""
        self._check(self.L.yams_accel_ctx_set_gate(self.ctx, gate.h if gate is not None else None))
        self._gate = gate

    # ---- misc ---------------------------------------------------------------------------------
    def device_info(self) -> dict:
        p = C.c_void_p()
        self._check(self.L.yams_accel_device_info_json(self.ctx, C.byref(p)))
        s = C.string_at(p).decode()
        self.L.yams_accel_free_string(p)
        return json.loads(s)

    def synchronize(self):
        self._check(self.L.yams_accel_ctx_synchronize(self.ctx))

    def alloc(self, nbytes: int) -> DeviceArray:
        return DeviceArray(self, nbytes)

    def to_device(self, arr: np.ndarray) -> DeviceArray:
        arr = np.ascontiguousarray(arr)
        return DeviceArray(self, max(arr.nbytes, 16)).upload(arr)

    def enable_timing(self, on: bool = True):
        self._check(self.L.yams_accel_enable_kernel_timing(self.ctx, 1 if on else 0))

    def kernel_ms(self, name: str):
        ms = C.c_double(0)
        n = C.c_uint64(0)
        st = self.L.yams_accel_last_kernel_ms(self.ctx, name.encode(), C.byref(ms), C.byref(n))
        if st == _lib.YAMS_ERR_NOT_FOUND:
            return None, 0
        self._check(st)
        return ms.value, n.value

    # ---- exact vector scan --------------------------------------------------------------------
    def corpus_view(self, rows_ptr: int, n_rows: int, dim: int, tie_rank_ptr: int | None = None,
                    rank_row_ptr: int | None = None, row_base: int = 0,
                    row_mask_ptr: int | None = None, row_mask_count: int = 0,
                    rows_bf16_ptr: int | None = None, rows_nsq_ptr: int | None = None,
                    rows_i8_ptr: int | None = None, rows_i8_meta_ptr: int | None = None,
                    stripe_rows: int = 0, n_stripes: int = 0, stripe_index: int = 0, i8_flags: int = 0) -> ScanCorpus:
        return ScanCorpus(rows_ptr, n_rows, dim, 0, tie_rank_ptr, rank_row_ptr, row_base,
                          row_mask_ptr, row_mask_count, rows_bf16_ptr, rows_nsq_ptr,
                          rows_i8_ptr, rows_i8_meta_ptr, stripe_rows, n_stripes, stripe_index, i8_flags)

    def build_shadow_device(self, rows_ptr: int, n_rows: int, dim: int, out_bf16_ptr: int,
                            out_nsq_ptr: int) -> None:
        """Filter shadow of the rows (bf16 RNE copy + fp32 squared norms); asynchronous."""
        self._check(self.L.yams_scan_build_shadow_device(self.ctx, rows_ptr, n_rows, dim,
                                                         out_bf16_ptr, out_nsq_ptr))

    def build_shadow_i8_device(self, rows_ptr: int, n_rows: int, dim: int, out_i8_ptr: int,
                               out_meta_ptr: int, want_mean_err: bool = False, first_row: int = 0, i8_flags: int = 0):
        """INT8 filter shadow of rows [first_row, first_row + n_rows) of the mirror whose arrays start
        at the given BASE pointers: int8 rows [n][dim] + {scale, residue bound} per block of 64 rows
        ([ceil(n / 64)][2] fp32), in the layout `i8_flags` names (the view must carry the same bits).
        Asynchronous unless the mean residue bound is asked for."""
        me = C.c_double(0.0)
        self._check(self.L.yams_scan_build_shadow_i8_layout_device(self.ctx, rows_ptr, first_row, n_rows, dim, i8_flags, out_i8_ptr,
                                                                   out_meta_ptr, C.byref(me) if want_mean_err else None))
        return me.value if want_mean_err else None

    def choose_i8_layout(self, rows_ptr: int, n_rows: int, dim: int):
        """(i8_flags, mean residue plain, mean residue rotated) measured on a sample of blocks; synchronises."""
        fl = C.c_uint32(0); a = C.c_double(0.0); b = C.c_double(0.0)
        self._check(self.L.yams_scan_choose_i8_layout_device(self.ctx, rows_ptr, n_rows, dim, C.byref(fl), C.byref(a), C.byref(b)))
        return fl.value, a.value, b.value

    def scan_topk_device(self, corpus: ScanCorpus, queries_ptr: int, nq: int, k: int,
                         threshold: float, metric: int, out_scores: int, out_rows: int,
                         out_counts: int, out_dist: int | None = None,
                         out_ranks: int | None = None, flags: int = 0, want_diag: bool = True):
        prm = ScanParams(k, threshold, metric, flags)
        diag = ScanDiag()
        self._check(self.L.yams_scan_topk_device(self.ctx, C.byref(corpus), queries_ptr, nq,
                                                 C.byref(prm), out_scores, out_rows, out_counts,
                                                 out_dist, out_ranks,
                                                 C.byref(diag) if want_diag else None))
        return diag.as_dict() if want_diag else None

    def scan_topk(self, corpus: ScanCorpus, queries: np.ndarray, k: int, threshold: float = 0.0,
                  metric: int = SCAN_COSINE, flags: int = 0) -> ScanResult:
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        kk = max(k, 1)
        scores = np.full((nq, kk), -np.inf, np.float32)
        rows = np.full((nq, kk), -1, np.int64)
        counts = np.zeros(nq, np.uint32)
        dist = np.full((nq, kk), np.inf, np.float32)
        prm = ScanParams(k, threshold, metric, flags)
        diag = ScanDiag()
        self._check(self.L.yams_scan_topk_host(self.ctx, C.byref(corpus), q.ctypes.data, nq,
                                               C.byref(prm), scores.ctypes.data, rows.ctypes.data,
                                               counts.ctypes.data, dist.ctypes.data,
                                               C.byref(diag)))
        return ScanResult(scores[:, :k], rows[:, :k], counts, dist[:, :k], diag.as_dict())

    def docs_view(self, row_doc_ptr: int, n_docs: int, doc_rank_ptr: int | None = None) -> ScanDocs:
        """yams_scan_docs_t over device arrays: row_doc u32 [n_rows] (NO_DOC = no document), doc_rank u32 [n_docs] or None."""
        return ScanDocs(row_doc_ptr, doc_rank_ptr, n_docs, 0)

    def scan_doc_topk(self, corpus: ScanCorpus, docs: ScanDocs, queries: np.ndarray, k: int, threshold: float = 0.0,
                      metric: int = SCAN_COSINE, flags: int = 0) -> ScanResult:
        """Document-level top-k (yams_scan_doc_topk_device) from host queries: the k best documents per query, each by its
        best row.  The result's `docs` holds the document ordinals, `matching` the rows >= threshold before the reduction."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        kk = max(k, 1)
        d_q = self.to_device(q) if q.size else None
        d_s = self.alloc(nq * kk * 4 + 16); d_r = self.alloc(nq * kk * 8 + 16); d_d = self.alloc(nq * kk * 4 + 16)
        d_n = self.alloc(nq * 4 + 16); d_m = self.alloc(nq * 8 + 16)
        try:
            prm = ScanParams(k, threshold, metric, flags)
            diag = ScanDiag()
            self._check(self.L.yams_scan_doc_topk_device(self.ctx, C.byref(corpus), C.byref(docs), d_q.ptr if d_q else None, nq,
                                                         C.byref(prm), d_s.ptr, d_r.ptr, d_d.ptr, d_n.ptr, d_m.ptr, C.byref(diag)))
            counts = d_n.download(np.uint32, nq)
            scores = d_s.download(np.float32, nq * kk).reshape(nq, kk)[:, :k]
            rows = d_r.download(np.int64, nq * kk).reshape(nq, kk)[:, :k]
            docs_out = d_d.download(np.uint32, nq * kk).reshape(nq, kk)[:, :k]
            matching = d_m.download(np.uint64, nq)
        finally:
            for b in (d_q, d_s, d_r, d_d, d_n, d_m):
                if b is not None:
                    b.free()
        if k == 0:
            scores = np.zeros((nq, 0), np.float32); rows = np.zeros((nq, 0), np.int64); docs_out = np.zeros((nq, 0), np.uint32)
        r = ScanResult(scores, rows, counts, None, diag.as_dict())
        r.docs = docs_out
        r.matching = matching
        return r

    def entities_view(self, row_type_ptr: int | None = None, row_node_type_ptr: int | None = None,
                      row_doc_ptr: int | None = None) -> "_lib.ScanEntities":
        """yams_scan_entities_t over device columns: row_type u8 [n_rows], row_node_type / row_doc u32 [n_rows] (each or None)."""
        return _lib.ScanEntities(row_type_ptr, row_node_type_ptr, row_doc_ptr)

    def scan_entity_topk(self, corpus: ScanCorpus, entities, queries: np.ndarray, k: int, threshold: float = 0.5,
                         filters=None) -> ScanResult:
        """IEntityStore::searchEntities on the device (yams_scan_entity_topk_device) from host queries.  filters: None, or one
        (embedding_type | None, node_type id | None, document id | None) per query.  The result's `matching` holds the rows
        kept by the threshold; zero / NaN / inf queries are served."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        kk = max(k, 1)
        fl = None
        if filters is not None:
            assert len(filters) == nq
            fl = (_lib.EntityFilter * max(nq, 1))()
            for i, (t, nt, d) in enumerate(filters):
                fl[i] = _lib.EntityFilter((_lib.ENTITY_FILTER_TYPE if t is not None else 0) | (_lib.ENTITY_FILTER_NODE_TYPE if nt is not None else 0) |
                                          (_lib.ENTITY_FILTER_DOC if d is not None else 0), t or 0, nt or 0, d or 0)
        d_q = self.to_device(q) if q.size else None
        d_s = self.alloc(nq * kk * 4 + 16); d_r = self.alloc(nq * kk * 8 + 16)
        d_n = self.alloc(nq * 4 + 16); d_m = self.alloc(nq * 8 + 16)
        try:
            diag = ScanDiag()
            self._check(self.L.yams_scan_entity_topk_device(self.ctx, C.byref(corpus), C.byref(entities), d_q.ptr if d_q else None, fl, nq,
                                                            k, threshold, d_s.ptr, d_r.ptr, d_n.ptr, d_m.ptr, C.byref(diag)))
            counts = d_n.download(np.uint32, nq)
            scores = d_s.download(np.float32, nq * kk).reshape(nq, kk)[:, :k]
            rows = d_r.download(np.int64, nq * kk).reshape(nq, kk)[:, :k]
            matching = d_m.download(np.uint64, nq)
        finally:
            for b in (d_q, d_s, d_r, d_n, d_m):
                if b is not None:
                    b.free()
        r = ScanResult(scores, rows, counts, None, diag.as_dict())
        r.matching = matching
        return r

    def _effective_k(self, n: int, k: int) -> int:
        kk = k if k else int(np.floor(np.sqrt(float(n)) + 0.5))
        return min(max(kk, 2), n)

    def cluster_kmeans_device(self, rows_ptr: int, n: int, dim: int, k: int = 0, max_iterations: int = 0,
                              membership_ptr: int | None = None, centroids_ptr: int | None = None):
        """yams_cluster_kmeans_device over device arrays; returns (k_eff, iterations run)."""
        ke = C.c_uint32(); it = C.c_uint32()
        self._check(self.L.yams_cluster_kmeans_device(self.ctx, rows_ptr, n, dim, k, max_iterations, membership_ptr, centroids_ptr,
                                                      C.byref(ke), C.byref(it)))
        return ke.value, it.value

    def cluster_kmeans(self, rows: np.ndarray, k: int = 0, max_iterations: int = 0, host_entry: bool = False):
        """The topology build's spherical k-means (runKMeans of engine kmeans_v1) of host rows [n][dim]: returns
        (membership [n] uint32, centroids [k_eff][dim] float32, k_eff, iterations run).  host_entry=True goes through
        yams_cluster_kmeans_host instead of uploading here."""
        x = np.ascontiguousarray(rows, dtype=np.float32)
        assert x.ndim == 2
        n, dim = x.shape
        if n == 0:
            ke, it = self.cluster_kmeans_device(None, 0, dim, k, max_iterations)
            return np.zeros(0, np.uint32), np.zeros((0, dim), np.float32), ke, it
        kmax = self._effective_k(n, k)
        ke = C.c_uint32(); it = C.c_uint32()
        mem, cent = self._artifact_call(
            self.L.yams_cluster_kmeans_device, self.L.yams_cluster_kmeans_host, host_entry,
            [x if x.size else None], [(np.uint32, n), (np.float32, kmax * dim)],
            lambda i, o: (i[0], n, dim, k, max_iterations, o[0], o[1], C.byref(ke), C.byref(it)))
        return mem, cent[:ke.value * dim].reshape(ke.value, dim), ke.value, it.value

    def cluster_assign(self, rows: np.ndarray, centroids: np.ndarray, empty: np.ndarray | None = None, with_distance: bool = True):
        """nearestCentroid of every host row over host centroids (yams_cluster_assign_device): (assign [n] uint32, distance
        [n] float64 or None).  empty: per-centroid flags of centroids to skip."""
        x = np.ascontiguousarray(rows, dtype=np.float32)
        n, dim = x.shape
        c = np.ascontiguousarray(centroids, dtype=np.float32).reshape(-1, dim) if dim else np.zeros((0, 0), np.float32)
        nc = c.shape[0]
        if n == 0:
            self._check(self.L.yams_cluster_assign_device(self.ctx, None, 0, dim, None, nc, None, None, None))
            return np.zeros(0, np.uint32), (np.zeros(0, np.float64) if with_distance else None)
        d_x = self.to_device(x) if x.size else None
        d_c = self.to_device(c) if c.size else None
        d_e = self.to_device(np.ascontiguousarray(empty, dtype=np.uint8)) if empty is not None and nc else None
        d_a = self.alloc(n * 4 + 16); d_d = self.alloc(n * 8 + 16) if with_distance else None
        try:
            self._check(self.L.yams_cluster_assign_device(self.ctx, d_x.ptr if d_x else None, n, dim, d_c.ptr if d_c else None, nc,
                                                          d_e.ptr if d_e else None, d_a.ptr, d_d.ptr if d_d else None))
            a = d_a.download(np.uint32, n)
            dist = d_d.download(np.float64, n) if d_d else None
        finally:
            for b in (d_x, d_c, d_e, d_a, d_d):
                if b is not None:
                    b.free()
        return a, dist

    def semantic_neighbors_device(self, rows_ptr: int, n: int, dim: int, k: int, out_rows_ptr: int, out_sims_ptr: int,
                                  out_counts_ptr: int, tie_rank_ptr: int | None = None, source_rows_ptr: int | None = None,
                                  n_sources: int = 0, threshold: float | None = None, out_inv_norm_ptr: int | None = None) -> dict:
        """yams_graph_semantic_neighbors_device over device arrays; threshold=None is the adaptive mode.  Returns the
        diagnostics {stripes, source_tiles, pairs_scored, pairs_admitted}."""
        diag = _lib.GraphDiag()
        flags = 0 if threshold is None else _lib.GRAPH_FLAG_EXPLICIT_THRESHOLD
        self._check(self.L.yams_graph_semantic_neighbors_device(self.ctx, rows_ptr, n, dim, tie_rank_ptr, source_rows_ptr, n_sources, k,
                                                                flags, 0.0 if threshold is None else threshold, out_rows_ptr,
                                                                out_sims_ptr, out_counts_ptr, out_inv_norm_ptr, C.byref(diag)))
        return diag.as_dict()

    def semantic_neighbors(self, rows: np.ndarray, k: int = 8, tie_rank: np.ndarray | None = None,
                           source_rows: np.ndarray | None = None, threshold: float | None = None, host_entry: bool = False):
        """The semantic-neighbour graph's pair loop (EmbeddingService::updateSemanticNeighborGraphUnlocked) over host rows
        [n][dim]: for every source (every row, or source_rows) its best k other rows.  Returns (rows [S][k] uint32 with
        0xffffffff in unused slots, sims [S][k] float32 with -inf there, counts [S] uint32, inv_norm [n] float32, diag).
        threshold=None is the adaptive mode (sim <= 0 dropped).  host_entry=True goes through
        yams_graph_semantic_neighbors_host instead of uploading here."""
        x = np.ascontiguousarray(rows, dtype=np.float32)
        assert x.ndim == 2
        n, dim = x.shape
        tr = None if tie_rank is None else np.ascontiguousarray(tie_rank, dtype=np.uint32)
        sr = None if source_rows is None else np.ascontiguousarray(source_rows, dtype=np.uint32)
        S = n if sr is None else len(sr)
        flags = 0 if threshold is None else _lib.GRAPH_FLAG_EXPLICIT_THRESHOLD
        thr = 0.0 if threshold is None else threshold
        diag = _lib.GraphDiag()

        def some(a):      # a list without entries still has to be an address: a null pointer means "every row" / "no ranks"
            return None if a is None else (a if a.size else np.zeros(1, a.dtype))
        o_r, o_s, o_c, o_i = self._artifact_call(
            self.L.yams_graph_semantic_neighbors_device, self.L.yams_graph_semantic_neighbors_host, host_entry,
            [x if x.size else None, some(tr), some(sr)], [(np.uint32, S * k), (np.float32, S * k), (np.uint32, S), (np.float32, n)],
            lambda i, o: (i[0], n, dim, i[1], i[2], S, k, flags, thr, o[0], o[1], o[2], o[3], C.byref(diag)))
        if not (k and n >= 2 and S):      # the entry writes nothing then: an empty result
            o_r[:] = 0xffffffff; o_s[:] = -np.inf; o_c[:] = 0; o_i[:] = 0
        return o_r.reshape(S, k), o_s.reshape(S, k), o_c, o_i, diag.as_dict()

    def semantic_neighbors_host(self, rows: np.ndarray, k: int = 8, **kw):
        """semantic_neighbors through yams_graph_semantic_neighbors_host (host arrays in, host arrays out)."""
        return self.semantic_neighbors(rows, k, host_entry=True, **kw)

    def sgc_smooth_device(self, rows_ptr: int, n: int, dim: int, row_offsets_ptr: int, cols_ptr: int | None, weights_ptr: int | None,
                          hops: int, out_ptr: int) -> dict:
        """yams_graph_sgc_smooth_device over device arrays.  Returns the diagnostics {nnz, edges_skipped_zero_scale,
        max_degree, hops, hub_rows}."""
        diag = _lib.SgcDiag()
        self._check(self.L.yams_graph_sgc_smooth_device(self.ctx, rows_ptr, n, dim, row_offsets_ptr, cols_ptr, weights_ptr, hops, out_ptr,
                                                        C.byref(diag)))
        return diag.as_dict()

    def sgc_smooth(self, rows: np.ndarray, row_offsets: np.ndarray, cols: np.ndarray, weights: np.ndarray, hops: int,
                   host_entry: bool = False):
        """SGC smoothing (applySGCSmoothing's degree pass and hop loop) of host rows [n][dim] over the list (row_offsets [n + 1]
        uint64, cols uint32, weights float32): the order of a row's edges is the order of its fp32 sums.  Returns (out [n][dim]
        float32, diag).  host_entry=True goes through yams_graph_sgc_smooth_host instead of uploading here."""
        x = np.ascontiguousarray(rows, dtype=np.float32)
        assert x.ndim == 2
        n, dim = x.shape
        off = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        c = np.ascontiguousarray(cols, dtype=np.uint32)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        diag = _lib.SgcDiag()
        out, = self._artifact_call(
            self.L.yams_graph_sgc_smooth_device, self.L.yams_graph_sgc_smooth_host, host_entry,
            [x if x.size else None, off, c if c.size else None, w if w.size else None], [(np.float32, x.size)],
            lambda i, o: (i[0], n, dim, i[1], i[2], i[3], hops, o[0], C.byref(diag)))
        return out.reshape(n, dim), diag.as_dict()

    # ---- cluster artifacts (yams_cluster_centroids / _representatives / _residuals) ----------------------------------------
    _GUARD = 0xA5

    def _artifact_call(self, fn_device, fn_host, host_entry: bool, inputs: list, outputs: list, build_args, misalign: int = 0, ctx=None):
        """Runs one artifact entry.  inputs: numpy arrays or None; outputs: (dtype, count) or None.  build_args(in_ptrs,
        out_ptrs) gives the argument tuple after ctx.  Device outputs are followed by 64 guard bytes that must come back
        untouched; misalign shifts every float input by that many bytes (float-aligned, not 16-byte-aligned bases).  ctx: the
        handle the entry takes first, when it is not the context."""
        ctx = self.ctx if ctx is None else ctx
        sizes = [None if o is None else np.dtype(o[0]).itemsize * o[1] for o in outputs]
        if host_entry:
            outs = [None if nb is None else np.full(nb + 64, self._GUARD, np.uint8) for nb in sizes]
            try:
                self._check(fn_host(ctx, *build_args([None if a is None else a.ctypes.data for a in inputs],
                                                          [None if o is None else o.ctypes.data for o in outs])))
            except AccelError:
                assert all(o is None or (o == self._GUARD).all() for o in outs), "a refused artifact call wrote to an output"
                raise
            assert all(o is None or (o[nb:] == self._GUARD).all() for o, nb in zip(outs, sizes)), "an artifact entry wrote behind its output"
            return [None if o is None else o[:nb].view(outputs[i][0]).copy() for i, (o, nb) in enumerate(zip(outs, sizes))]
        bufs, in_ptrs = [], []
        try:
            for a in inputs:
                if a is None:
                    in_ptrs.append(None)
                    continue
                shift = misalign if a.dtype == np.float32 else 0
                b = self.alloc(a.nbytes + 32)
                b.upload(a, shift)
                bufs.append(b)
                in_ptrs.append(b.ptr + shift)
            out_bufs = []
            for o in outputs:
                if o is None:
                    out_bufs.append(None)
                    continue
                nbytes = np.dtype(o[0]).itemsize * o[1]
                b = self.alloc(nbytes + 64)
                b.upload(np.full(nbytes + 64, self._GUARD, np.uint8))
                bufs.append(b)
                out_bufs.append(b)
            try:
                self._check(fn_device(ctx, *build_args(in_ptrs, [None if b is None else b.ptr for b in out_bufs])))
            except AccelError:      # a refusal writes nothing: the outputs and the guard bytes behind them are as they were
                for b in out_bufs:
                    assert b is None or (b.download(np.uint8, b.nbytes) == self._GUARD).all(), "a refused artifact call wrote to an output"
                raise
            res = []
            for o, b in zip(outputs, out_bufs):
                if o is None:
                    res.append(None)
                    continue
                nbytes = np.dtype(o[0]).itemsize * o[1]
                raw = b.download(np.uint8, nbytes + 64)
                assert (raw[nbytes:] == self._GUARD).all(), "an artifact entry wrote behind its output"
                res.append(raw[:nbytes].view(o[0]).copy())
            return res
        finally:
            for b in bufs:
                b.free()

    def cluster_centroids(self, rows: np.ndarray, cluster_offsets, members, host_entry: bool = False, misalign: int = 0):
        """meanEmbedding of every cluster (yams_cluster_centroids_device / _host): rows [n][dim] float32, CSR member lists in
        the order of the sums.  Returns (centroids [c][dim] float32, counts [c] uint32)."""
        x = np.ascontiguousarray(rows, np.float32)
        n, dim = x.shape
        off = np.ascontiguousarray(cluster_offsets, np.uint64)
        mem = np.ascontiguousarray(members, np.uint32)
        c = len(off) - 1
        cent, cnt = self._artifact_call(
            self.L.yams_cluster_centroids_device, self.L.yams_cluster_centroids_host, host_entry,
            [x if x.size else None, off, mem if mem.size else None], [(np.float32, c * dim), (np.uint32, c)],
            lambda i, o: (i[0], n, dim, i[1], i[2], c, o[0], o[1]), misalign)
        return cent.reshape(c, dim), cnt

    def cluster_representatives(self, rows: np.ndarray, cluster_offsets, candidates, centroids: np.ndarray, n_extra: int,
                                centroid_empty=None, host_entry: bool = False, misalign: int = 0):
        """The selection loop of selectDiverseRoutingRepresentatives for every cluster (yams_cluster_representatives_device /
        _host).  Returns (selected [c][n_extra] uint32 positions in the candidate lists, 0xffffffff = unused; counts [c])."""
        x = np.ascontiguousarray(rows, np.float32)
        n, dim = x.shape
        off = np.ascontiguousarray(cluster_offsets, np.uint64)
        cand = np.ascontiguousarray(candidates, np.uint32)
        cen = np.ascontiguousarray(centroids, np.float32)
        c = len(off) - 1
        emp = None if centroid_empty is None else np.ascontiguousarray(centroid_empty, np.uint8)
        sel, cnt = self._artifact_call(
            self.L.yams_cluster_representatives_device, self.L.yams_cluster_representatives_host, host_entry,
            [x if x.size else None, off, cand if cand.size else None, cen if cen.size else None, emp],
            [(np.uint32, c * n_extra), (np.uint32, c)],
            lambda i, o: (i[0], n, dim, i[1], i[2], i[3], i[4], c, n_extra, o[0], o[1]), misalign)
        return sel.reshape(c, n_extra), cnt

    def cluster_residuals(self, rows: np.ndarray, centroids: np.ndarray, primary=None, cand_offsets=None, cand=None,
                          form: int = _lib.RESIDUAL_SEPARATE, host_entry: bool = False, misalign: int = 0):
        """The chains of applyOrthogonalBoundarySpill (yams_cluster_residuals_device / _host).  primary [n] uint32 or None
        (0xffffffff = none); cand_offsets / cand: CSR candidate lists, or None for every cluster in index order.  Returns
        (primary_norm_sq [n] or None, cand_norm_sq [pairs], residual_dot [pairs] or None), float64."""
        x = np.ascontiguousarray(rows, np.float32)
        n, dim = x.shape
        cen = np.ascontiguousarray(centroids, np.float32).reshape(-1, dim)
        c = cen.shape[0]
        pri = None if primary is None else np.ascontiguousarray(primary, np.uint32)
        off = None if cand_offsets is None else np.ascontiguousarray(cand_offsets, np.uint64)
        lst = None if cand is None else np.ascontiguousarray(cand, np.uint32)
        pairs = int(off[-1]) if off is not None else n * c
        if lst is not None and lst.size == 0:
            lst = np.zeros(1, np.uint32)
        pn, cn, rd = self._artifact_call(
            self.L.yams_cluster_residuals_device, self.L.yams_cluster_residuals_host, host_entry,
            [x if x.size else None, cen if cen.size else None, pri, off, lst],
            [(np.float64, n) if pri is not None else None, (np.float64, pairs), (np.float64, pairs) if pri is not None else None],
            lambda i, o: (i[0], n, dim, i[1], c, i[2], i[3], i[4], form, o[0], o[1], o[2]), misalign)
        return pn, cn, rd

    # ---- topological quality (yams_quality_persistence_h0_*) --------------------------------------------------------------
    def persistence_h0(self, rows: np.ndarray, select=None, form: int = _lib.RESIDUAL_SEPARATE, host_entry: bool = False,
                       want_distances: bool = False, want_weights: bool = False, misalign: int = 0):
        """computePersistenceH0 of the points rows[select] (all rows without select): yams_quality_persistence_h0_device /
        _host.  Returns a dict: value, norm, norm_index, n_edges, n_points, n_merges and, when asked for, distances [m][m]
        float64, weights [m - 1] float64 ascending."""
        x = np.ascontiguousarray(rows, np.float32)
        n, dim = x.shape
        sel = None if select is None else np.ascontiguousarray(select, np.uint32)
        m = n if sel is None else len(sel)
        res = _lib.PersistenceH0()
        if sel is not None and sel.size == 0:
            sel = np.zeros(1, np.uint32)
        dist, w = self._artifact_call(
            self.L.yams_quality_persistence_h0_device, self.L.yams_quality_persistence_h0_host, host_entry,
            [x if x.size else None, sel], [(np.float64, m * m) if want_distances else None, (np.float64, max(m - 1, 0)) if want_weights else None],
            lambda i, o: (i[0], n, dim, i[1], m, form, C.byref(res), o[0], o[1], None), misalign)
        out = {k: getattr(res, k) for k, _ in _lib.PersistenceH0._fields_}
        if want_distances:
            out["distances"] = dist.reshape(m, m)
        if want_weights:
            out["weights"] = w
        return out

    # ---- topology input features (yams_features_*) -----------------------------------------------------------------------------
    def features_aggregate(self, rows: np.ndarray, doc_offsets, records, host_entry: bool = False, misalign: int = 0):
        """aggregateEmbedding of every document (yams_features_aggregate_device / _host): rows [n_records][dim] float32, CSR
        record lists in the order of the sums.  Returns (out [n_docs][dim] float32, counts [n_docs] uint32)."""
        x = np.ascontiguousarray(rows, np.float32)
        n, dim = x.shape
        off = np.ascontiguousarray(doc_offsets, np.uint64)
        rec = np.ascontiguousarray(records, np.uint32)
        d = len(off) - 1
        out, cnt = self._artifact_call(
            self.L.yams_features_aggregate_device, self.L.yams_features_aggregate_host, host_entry,
            [x if x.size else None, off, rec if rec.size else None], [(np.float32, d * dim), (np.uint32, d)],
            lambda i, o: (i[0], n, dim, i[1], i[2], d, o[0], o[1]), misalign)
        return out.reshape(d, dim), cnt

    def features_variance(self, rows: np.ndarray, select=None, form: int = _lib.RESIDUAL_SEPARATE, host_entry: bool = False,
                          misalign: int = 0):
        """The two passes of computeVarianceWeights over rows[select] in order (all rows without select):
        yams_features_variance_device / _host.  Returns (mean [dim], var [dim]) float64, or (None, None) when m == 0 (nothing
        is written then: the guard words are checked)."""
        x = np.ascontiguousarray(rows, np.float32)
        n, dim = x.shape
        sel = None if select is None else np.ascontiguousarray(select, np.uint32)
        m = n if sel is None else len(sel)
        if sel is not None and sel.size == 0:
            sel = np.zeros(1, np.uint32)
        if m == 0:      # written nowhere: every byte of the outputs must still be the guard
            guard = self._GUARD
            mean, var = self._artifact_call(
                self.L.yams_features_variance_device, self.L.yams_features_variance_host, host_entry,
                [x if x.size else None, sel], [(np.uint8, dim * 8), (np.uint8, dim * 8)],
                lambda i, o: (i[0], n, dim, i[1], m, form, o[0], o[1]), misalign)
            assert (mean == guard).all() and (var == guard).all(), "m == 0 wrote to an output"
            return None, None
        mean, var = self._artifact_call(
            self.L.yams_features_variance_device, self.L.yams_features_variance_host, host_entry,
            [x if x.size else None, sel], [(np.float64, dim), (np.float64, dim)],
            lambda i, o: (i[0], n, dim, i[1], m, form, o[0], o[1]), misalign)
        return mean, var

    def features_compose(self, dense: np.ndarray, weights=None, entity=None, entity_on=None, sig=None, sketch_on=None,
                         sketch_dim: int = 0, alpha_e: float = 0.0, alpha_m: float = 0.0, out_stride=None, host_entry: bool = False,
                         misalign: int = 0):
        """composeFeatureVector of every row (yams_features_compose_device / _host).  weights [dim] float32 or None (host
        memory in both twins); entity [n][K] float32 or None; sig [n][sig_len] uint32 or None.  Returns (out [n][out_stride]
        float32, dims [n] uint32); out_stride defaults to the longest possible row."""
        x = np.ascontiguousarray(dense, np.float32)
        n, dim = x.shape
        w = None if weights is None else np.ascontiguousarray(weights, np.float32)
        ent = None if entity is None else np.ascontiguousarray(entity, np.float32)
        eon = None if entity_on is None else np.ascontiguousarray(entity_on, np.uint8)
        sg = None if sig is None else np.ascontiguousarray(sig, np.uint32)
        son = None if sketch_on is None else np.ascontiguousarray(sketch_on, np.uint8)
        k = 0 if ent is None else ent.shape[1]
        sig_len = 0 if sg is None else sg.shape[1]
        if out_stride is None:
            kc = dim if w is None else int((w > 0).sum())
            out_stride = kc + (k if ent is not None else 0) + (sketch_dim if sg is not None and sig_len and sketch_dim else 0)

        def some(a):      # an array without elements still has to be an address
            return None if a is None else (a if a.size else np.zeros(4, a.dtype))
        out, dims = self._artifact_call(
            self.L.yams_features_compose_device, self.L.yams_features_compose_host, host_entry,
            [x if x.size else None, some(ent), some(eon), some(sg), some(son)], [(np.float32, n * out_stride), (np.uint32, n)],
            lambda i, o: (i[0], n, dim, None if w is None else w.ctypes.data, i[1], k, i[2], i[3], sig_len, i[4], sketch_dim, alpha_e,
                          alpha_m, o[0], out_stride, o[1]), misalign)
        return out.reshape(n, out_stride), dims

    # ---- late-interaction rerank (yams_rerank_*) ----------------------------------------------------------------------------------
    def rerank_maxsim(self, query: np.ndarray, rows: np.ndarray, doc_offsets, form: int = _lib.RESIDUAL_SEPARATE, want_rowmax: bool = False,
                      host_entry: bool = False, misalign: int = 0):
        """computeMaxSim of every document of a window (yams_rerank_maxsim_device / _host): query [tq][dim] float32, rows
        [total][dim] float32, CSR documents.  Returns (scores [n_docs] float32, diag dict) or, with want_rowmax, (scores, rowmax
        [n_docs][tq] float32, rowarg [n_docs][tq] uint32, diag)."""
        q = np.ascontiguousarray(query, np.float32)
        x = np.ascontiguousarray(rows, np.float32)
        tq, dim = q.shape
        off = np.ascontiguousarray(doc_offsets, np.uint64)
        d = len(off) - 1
        dg = _lib.RerankDiag()
        outs = [(np.float32, d), (np.float32, d * tq) if want_rowmax else None, (np.uint32, d * tq) if want_rowmax else None]
        sc, mx, arg = self._artifact_call(
            self.L.yams_rerank_maxsim_device, self.L.yams_rerank_maxsim_host, host_entry,
            [q if q.size else None, x if x.size else None, off], outs,
            lambda i, o: (i[0], tq, dim, i[1], i[2], d, form, o[0], o[1], o[2], C.byref(dg)), misalign)
        diag = {k: getattr(dg, k) for k, _ in _lib.RerankDiag._fields_}
        if want_rowmax:
            return sc, mx.reshape(d, tq), arg.reshape(d, tq), diag
        return sc, diag

    def rerank_maxpool(self, rows: np.ndarray, doc_offsets, host_entry: bool = False, misalign: int = 0):
        """normalizeEmbedding(maxPoolEmbeddings(document)) of every document (yams_rerank_maxpool_device / _host).  Returns out
        [n_docs][dim] float32."""
        x = np.ascontiguousarray(rows, np.float32)
        dim = x.shape[1]
        off = np.ascontiguousarray(doc_offsets, np.uint64)
        d = len(off) - 1
        out, = self._artifact_call(
            self.L.yams_rerank_maxpool_device, self.L.yams_rerank_maxpool_host, host_entry,
            [x if x.size else None, off], [(np.float32, d * dim)],
            lambda i, o: (i[0], dim, i[1], d, o[0]), misalign)
        return out.reshape(d, dim)

    # ---- the embedding model's pooling head (yams_embed_*) -----------------------------------------------------------------------
    def embed_pool(self, hidden: np.ndarray, mask=None, mode: int = _lib.EMBED_POOL_MEAN, normalize: bool = True, host_entry: bool = False,
                   misalign: int = 0):
        """The pooled row of every text (yams_embed_pool_device / _host): hidden [batch][seq][dim] float32, mask [batch][mask_len]
        int32 or None.  Returns (out [batch][dim] float32, diag dict)."""
        x = np.ascontiguousarray(hidden, np.float32)
        batch, seq, dim = x.shape
        m = None if mask is None else np.ascontiguousarray(mask, np.int32).reshape(batch, -1)
        mask_len = 0 if m is None else m.shape[1]
        flags = _lib.EMBED_NORMALIZE if normalize else 0
        dg = _lib.EmbedDiag()
        out, = self._artifact_call(
            self.L.yams_embed_pool_device, self.L.yams_embed_pool_host, host_entry,
            [x if x.size else None, m if m is not None and m.size else None], [(np.float32, batch * dim)],
            lambda i, o: (i[0], batch, seq, dim, i[1], mask_len, mode, flags, o[0], C.byref(dg)), misalign)
        return out.reshape(batch, dim), {k: getattr(dg, k) for k, _ in _lib.EmbedDiag._fields_}

    def embed_normalize(self, rows: np.ndarray, host_entry: bool = False, misalign: int = 0):
        """The rank-2 output: every row L2-normalised (yams_embed_normalize_device / _host).  Returns out [batch][dim] float32."""
        x = np.ascontiguousarray(rows, np.float32)
        batch, dim = x.shape
        out, = self._artifact_call(
            self.L.yams_embed_normalize_device, self.L.yams_embed_normalize_host, host_entry,
            [x if x.size else None], [(np.float32, batch * dim)], lambda i, o: (i[0], batch, dim, o[0]), misalign)
        return out.reshape(batch, dim)

    # ---- cluster routing (yams_route_index_* / yams_route_dense_*) ----------------------------------------------------------
    def route_index(self, vectors: np.ndarray, cluster_offsets, has_centroid, position, host_entry: bool = False,
                    misalign: int = 0) -> "RouteIndex":
        """The resident table of cluster vectors (yams_route_index_create_device / _host): vectors [v][dim] float32, cluster
        after cluster, the centroid first where has_centroid says so; position [v] uint16 = a representative's place in the
        reference's list.  The row norms come back as `.norms`."""
        return RouteIndex(self, vectors, cluster_offsets, has_centroid, position, host_entry, misalign)

    def route_dense(self, index: "RouteIndex", queries: np.ndarray, rep_limit: int = 0, candidates=None, host_entry: bool = False,
                    misalign: int = 0):
        """The dense signal of every query against the index (yams_route_dense_device / _host).  candidates: None or a bool
        array [q][c].  Returns (dense [q][c] float32, observed [q][c] bool, evaluations [q] uint32, diag dict)."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, index.dim)
        nq, c = q.shape[0], index.n_clusters
        bits = None
        if candidates is not None:
            bits = pack_candidates(np.asarray(candidates, bool).reshape(nq, c))
        diag = _lib.RouteDiag()
        dense, obs, ev = self._artifact_call(
            self.L.yams_route_dense_device, self.L.yams_route_dense_host, host_entry,
            [q if q.size else None, bits if bits is not None and bits.size else None],
            [(np.float32, nq * c), (np.uint8, nq * c), (np.uint32, nq)],
            lambda i, o: (i[0], nq, rep_limit, i[1], o[0], o[1], o[2], C.byref(diag)), misalign, ctx=index.h)
        return dense.reshape(nq, c), obs.reshape(nq, c).astype(bool), ev, {"pairs": diag.pairs, "slices": diag.slices, "form": diag.form}

    def scan_pq_topk(self, corpus: ScanCorpus, codes: np.ndarray, luts: np.ndarray, queries: np.ndarray, k: int, threshold: float = -1.0,
                     rerank_factor: int = 2, tie_keys: np.ndarray | None = None, row_of_index: np.ndarray | None = None,
                     candidates: np.ndarray | None = None, sum_lanes: int = 1, sum_flags: int | None = None) -> ScanResult:
        """The product-quantised engine's search (yams_scan_pq_topk_device; simeonPqSearchUnlocked, sqlite_vec_backend.cpp:
        3868-4056) from host arrays: codes u8 [n][m], luts f32 [nq][m][256] (what simeon's PQInnerProductQuery holds), raw
        queries [nq][dim], tie_keys u64 [n] (stableStringKey of the chunk ids), row_of_index u32 [n] (index -> corpus row),
        candidates: ascending indices or None.  The tie ranks and the key -> row table are derived here, as a host does once
        per index build.  The order of the ADC sum: sum_lanes (1 / 4 / 8 / 16 lanes, added left to right), or sum_flags, a whole
        YAMS_PQ_SUM_* word (lanes | combine | tail) that is passed as is and takes precedence."""
        codes = np.ascontiguousarray(codes, np.uint8)
        n, m = codes.shape
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        luts = np.ascontiguousarray(luts, np.float32).reshape(nq, m, 256)
        keep = []
        d_codes = self.to_device(codes); keep.append(d_codes)
        d_tie = d_keyrow = None
        order = None
        if tie_keys is not None:
            tk = np.ascontiguousarray(tie_keys, np.uint64)
            order = np.lexsort((np.arange(n), tk))            # ascending key, equal keys by index
            rank = np.empty(n, np.uint32); rank[order] = np.arange(n, dtype=np.uint32)
            d_tie = self.to_device(rank); keep.append(d_tie)
        if tie_keys is not None or row_of_index is not None:
            roi = np.arange(n, dtype=np.uint32) if row_of_index is None else np.ascontiguousarray(row_of_index, np.uint32)
            key_row = roi[order] if order is not None else roi  # key index r -> row of the code with that key index
            d_keyrow = self.to_device(np.ascontiguousarray(key_row, np.uint32)); keep.append(d_keyrow)
        pq = _lib.ScanPqIndex(d_codes.ptr, n, m, 0, d_tie.ptr if d_tie else None, d_keyrow.ptr if d_keyrow else None)
        d_q = self.to_device(q); d_l = self.to_device(luts); keep += [d_q, d_l]
        d_c = None; n_c = 0
        if candidates is not None:
            cand = np.ascontiguousarray(candidates, np.uint32)
            n_c = cand.size
            d_c = self.to_device(cand if n_c else np.zeros(1, np.uint32)); keep.append(d_c)
        kk = max(k, 1)
        d_s = self.alloc(nq * kk * 4); d_r = self.alloc(nq * kk * 8); d_n = self.alloc(nq * 4)
        prm = _lib.ScanPqParams(k, threshold, rerank_factor, {1: 0, 4: 1, 8: 2, 16: 3}[sum_lanes] if sum_flags is None else int(sum_flags))
        diag = ScanDiag()
        try:
            self._check(self.L.yams_scan_pq_topk_device(self.ctx, C.byref(corpus), C.byref(pq), d_q.ptr, d_l.ptr, nq, C.byref(prm),
                                                        d_c.ptr if d_c else None, n_c, d_s.ptr, d_r.ptr, d_n.ptr, C.byref(diag)))
            counts = d_n.download(np.uint32, nq)
            scores = d_s.download(np.float32, nq * kk).reshape(nq, kk)
            rows = d_r.download(np.int64, nq * kk).reshape(nq, kk)
        finally:
            for b in keep + [d_s, d_r, d_n]:
                b.free()
        return ScanResult(scores[:, :k], rows[:, :k], counts, None, diag.as_dict())

    def merge_topk_device(self, n_shards, nq, k, threshold, metric, in_scores, in_rows, in_counts,
                          in_dist, in_ranks, out_scores, out_rows, out_counts, out_dist, flags: int = 0):
        prm = ScanParams(k, threshold, metric, flags)
        self._check(self.L.yams_scan_merge_topk_device(self.ctx, n_shards, nq, C.byref(prm),
                                                       in_scores, in_rows, in_counts, in_dist,
                                                       in_ranks, out_scores, out_rows, out_counts,
                                                       out_dist))

    def record_layout(self, nq: int, k: int, with_dist: bool, with_ranks: bool) -> "_lib.RecordLayout":
        """yams_scan_record_layout: the offsets of one packed per-shard record (an absent part has offset 2**64 - 1)."""
        lay = _lib.RecordLayout()
        self.L.yams_scan_record_layout(nq, k, 1 if with_dist else 0, 1 if with_ranks else 0, C.byref(lay))
        return lay

    def merge_records_device(self, n_shards, nq, k, threshold, metric, records, record_stride, layout,
                             rank_of_row, rank_row_base, out_scores, out_rows, out_counts, out_dist, flags: int = 0):
        """yams_scan_merge_records_device over `n_shards` packed records `record_stride` bytes apart (device pointers)."""
        prm = ScanParams(k, threshold, metric, flags)
        self._check(self.L.yams_scan_merge_records_device(self.ctx, n_shards, nq, C.byref(prm), records, record_stride,
                                                          C.byref(layout) if layout is not None else None, rank_of_row,
                                                          rank_row_base, out_scores, out_rows, out_counts, out_dist))

    def synth_rows(self, seed: int, row0: int, n_rows: int, dim: int, out_ptr: int):
        self._check(self.L.yams_synth_rows_device(self.ctx, seed, row0, n_rows, dim, out_ptr))

    def synth_bytes(self, seed: int, blob0: int, n_blobs: int, blob_len: int, out_ptr: int):
        self._check(self.L.yams_synth_bytes_device(self.ctx, seed, blob0, n_blobs, blob_len, out_ptr))

    # ---- SHA-256 ------------------------------------------------------------------------------
    def sha256_hex(self, data: bytes | np.ndarray) -> str:
        a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else \
            np.ascontiguousarray(data, np.uint8)
        out = C.create_string_buffer(65)
        self._check(self.L.yams_sha256_host(self.ctx, a.ctypes.data if a.size else None, a.size, out))
        return out.value.decode()

    def sha256_many(self, msgs: list) -> list[str]:
        arrs = [np.frombuffer(bytes(m), np.uint8) if not isinstance(m, np.ndarray)
                else np.ascontiguousarray(m, np.uint8) for m in msgs]
        n = len(arrs)
        if n == 0:
            return []
        ptrs = (C.c_void_p * n)(*[a.ctypes.data if a.size else None for a in arrs])
        lens = (C.c_size_t * n)(*[a.size for a in arrs])
        out = C.create_string_buffer(65 * n)
        self._check(self.L.yams_sha256_many_host(self.ctx, ptrs, lens, n, out))
        raw = out.raw
        return [raw[65 * i:65 * i + 64].decode() for i in range(n)]

    def sha256_batch_device(self, data_ptr, offsets_ptr, lengths_ptr, n, digests_ptr):
        self._check(self.L.yams_sha256_batch_device(self.ctx, data_ptr, offsets_ptr, lengths_ptr,
                                                    n, digests_ptr))

    # ---- CRC-32 (the compressed store's header checksum) ------------------------------------------------
    def crc32_combine(self, crc_a: int, crc_b: int, len_b: int) -> int:
        return int(self.L.yams_crc32_combine(crc_a, crc_b, len_b))

    def crc32_many(self, msgs: list) -> np.ndarray:
        """yams_crc32_many_host: CRC-32 of every message (bytes / uint8 arrays / None for an empty one) -> uint32[n]."""
        arrs = [np.zeros(0, np.uint8) if m is None else np.frombuffer(bytes(m), np.uint8) if not isinstance(m, np.ndarray)
                else np.ascontiguousarray(m, np.uint8) for m in msgs]
        n = len(arrs)
        out = np.zeros(n, np.uint32)
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
        lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
        self._check(self.L.yams_crc32_many_host(self.ctx, ptrs, lens, n, out.ctypes.data_as(_lib.u32p)))
        return out

    def crc32(self, data) -> int:
        return int(self.crc32_many([data])[0])

    def crc32_batch_device(self, data_ptr, offsets_ptr, lengths_ptr, n, out_ptr):
        self._check(self.L.yams_crc32_batch_device(self.ctx, data_ptr, offsets_ptr, lengths_ptr, n, out_ptr))

    def crc32_chunks_device(self, data_ptr, blob_offsets, res: IngestResult, out_ptr, select_ptr=None):
        """The chunks of an ingest result over the same data and blob offsets; select_ptr: device u8[n_chunks] or None."""
        bo = np.ascontiguousarray(blob_offsets, np.uint64)
        self._check(self.L.yams_crc32_chunks_device(self.ctx, data_ptr, bo.ctypes.data_as(_lib.u64p), bo.size, C.byref(res),
                                                    select_ptr, out_ptr))

    def crc32_verify_device(self, data_ptr, offsets_ptr, lengths_ptr, n, expected_ptr, valid_ptr) -> int:
        """out_valid[i] = (crc == expected[i]); returns the number of mismatching messages."""
        bad = C.c_uint64(0)
        self._check(self.L.yams_crc32_verify_device(self.ctx, data_ptr, offsets_ptr, lengths_ptr, n, expected_ptr, valid_ptr,
                                                    C.byref(bad)))
        return bad.value

    # ---- chunking / ingest ----------------------------------------------------------------------
    def verify_chunks_device(self, data_ptr, offsets_ptr, lengths_ptr, n, expected_ptr, valid_ptr) -> int:
        """Batched integrity check; returns the number of mismatching chunks."""
        bad = C.c_uint64(0)
        self._check(self.L.yams_verify_chunks_device(self.ctx, data_ptr, offsets_ptr, lengths_ptr, n,
                                                     expected_ptr, valid_ptr, C.byref(bad)))
        return bad.value

    def dedup_set(self, expected_entries: int = 0) -> "DedupSet":
        return DedupSet(self, expected_entries)

    def chunk(self, data, cfg: CdcConfig | None = None, with_hashes: bool = True, context_len: int = 0):
        """IChunker::chunkDataLazy over host memory -> (offsets, sizes, hex hashes | None).  context_len > 0: one window
        of a stream (yams_cdc_chunk_window_host) — the leading bytes are history, chunks start behind them."""
        cfg = cfg or cdc_config()
        a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else \
            np.ascontiguousarray(data, np.uint8)
        floor = max(1, int(cfg.min_size))
        cap = a.size // floor + 2
        off = np.zeros(cap, np.uint64)
        sz = np.zeros(cap, np.uint64)
        hexbuf = C.create_string_buffer(65 * cap) if with_hashes else None
        cnt = C.c_size_t(0)
        self._check(self.L.yams_cdc_chunk_window_host(self.ctx, a.ctypes.data if a.size else None, a.size, context_len,
                                                      C.byref(cfg), off.ctypes.data_as(_lib.u64p),
                                                      sz.ctypes.data_as(_lib.u64p), hexbuf, cap,
                                                      C.byref(cnt)))
        n = cnt.value
        hashes = None
        if with_hashes:
            raw = hexbuf.raw
            hashes = [raw[65 * i:65 * i + 64].decode() for i in range(n)]
        return off[:n].copy(), sz[:n].copy(), hashes

    def ingest_device(self, data_ptr: int, blob_offsets, blob_lengths, cfg: CdcConfig | None = None,
                      flags: int = 3) -> IngestResult:
        cfg = cfg or cdc_config()
        bo = np.ascontiguousarray(blob_offsets, np.uint64)
        bl = np.ascontiguousarray(blob_lengths, np.uint64)
        res = IngestResult()
        self._check(self.L.yams_ingest_device(self.ctx, data_ptr, bo.ctypes.data_as(_lib.u64p),
                                              bl.ctypes.data_as(_lib.u64p), bo.size, C.byref(cfg),
                                              flags, C.byref(res)))
        return res

    def ingest_host(self, blob_ptrs, blob_lengths, cfg: CdcConfig | None = None, flags: int = 3,
                    batch_bytes: int = 0, chunk_cap: int | None = None, with_crc32: bool = False) -> dict:
        """yams_ingest_host: blobs in host memory (addresses in blob_ptrs), streamed through the device
        in batches.  Returns blob_first, chunk_offset, chunk_size, chunk_digest, blob_digest (numpy).
        with_crc32: yams_ingest_host_crc32 — the same call plus chunk_crc32 (uint32 per chunk)."""
        cfg = cfg or cdc_config()
        bl = np.ascontiguousarray(blob_lengths, np.uint64)
        n = int(bl.size)
        ptrs = (C.c_void_p * max(n, 1))(*[int(p) if p else None for p in blob_ptrs])
        if chunk_cap is None:
            chunk_cap = int(sum(int(x) // max(int(cfg.min_size), 1) + 2 for x in bl))
        first = np.zeros(n + 1, np.uint64)
        off = np.empty(chunk_cap, np.uint64); sz = np.empty(chunk_cap, np.uint64)
        dg = np.empty((chunk_cap, 32), np.uint8) if flags & 1 else None
        bd = np.empty((n, 32), np.uint8) if flags & 2 else None
        cnt = C.c_uint64(0)
        args = [self.ctx, ptrs, bl.ctypes.data_as(_lib.u64p), n, C.byref(cfg), flags, batch_bytes,
                first.ctypes.data_as(_lib.u64p), off.ctypes.data_as(_lib.u64p),
                sz.ctypes.data_as(_lib.u64p), dg.ctypes.data if dg is not None else None,
                chunk_cap, bd.ctypes.data if bd is not None else None, C.byref(cnt)]
        crc = np.empty(chunk_cap, np.uint32) if with_crc32 else None
        rc = self.L.yams_ingest_host_crc32(*args, crc.ctypes.data) if with_crc32 else self.L.yams_ingest_host(*args)
        self.last_required_chunks = int(cnt.value)
        self._check(rc)
        m = int(cnt.value)
        out = {"n_chunks": m, "blob_first": first, "chunk_offset": off[:m], "chunk_size": sz[:m],
               "chunk_digest": dg[:m] if dg is not None else None, "blob_digest": bd}
        if with_crc32:
            out["chunk_crc32"] = crc[:m]
        return out

    def download(self, ptr: int, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            self._check(self.L.yams_accel_download(self.ctx, out.ctypes.data, ptr, out.nbytes))
        return out

    def fetch_ingest(self, res: IngestResult, n_blobs: int) -> dict:
        n = res.n_chunks
        out = {"n_chunks": n,
               "chunk_offset": self.download(res.chunk_offset, np.uint64, n),
               "chunk_size": self.download(res.chunk_size, np.uint64, n),
               "chunk_blob": self.download(res.chunk_blob, np.uint32, n),
               "blob_first": self.download(res.blob_first, np.uint64, n_blobs + 1)}
        if res.chunk_digest:
            out["chunk_digest"] = self.download(res.chunk_digest, np.uint8, n * 32).reshape(n, 32)
        if res.blob_digest:
            out["blob_digest"] = self.download(res.blob_digest, np.uint8, n_blobs * 32).reshape(n_blobs, 32)
        return out
