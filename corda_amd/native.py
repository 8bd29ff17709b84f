"""ctypes binding of the C-ABI in include/cordaverify.h (corda_amd/libcordaverify.so).

This is the product path: there is no CPU fallback.  If the library is missing or no GPU is
present, the calls raise `NativeUnavailable` — loudly — instead of computing anything elsewhere.
"""
from __future__ import annotations

import ctypes
import os
import threading
import weakref
from typing import Optional, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# CV_LIB_PATH: load an alternative build of the same ABI (A/B tooling)
LIB_PATH = os.environ.get("CV_LIB_PATH") or os.path.join(HERE, "libcordaverify.so")

CV_OK = 0
CV_SIG_OK = 0
CV_SIG_BAD_KEY = 1
CV_TX_OK = 0
CV_TX_EMPTY = 1
CV_PMT_OK = 0
CV_PMT_EMPTY = 1
CV_PMT_MALFORMED = 2
CV_PMT_NOT_IN_TREE = 3
CV_PMT_NO_INCLUDED = 4
CV_UNIQ_OK = 0
CV_UNIQ_CONFLICT = 1
CV_UNIQ_SKIPPED = 2
CV_CK_LEAF = 0
CV_CK_NODE = 1
CV_VS_OK = 0
CV_VS_BAD_SIGNATURE = 1
CV_VS_MISSING = 2
CV_VS_MALFORMED = 3
# cv_notarise_batch outcome[t] (CV_NS_*)
CV_NS_SUCCESS, CV_NS_EMPTY, CV_NS_ID_MISMATCH, CV_NS_TIMESTAMP_INVALID, CV_NS_TX_INVALID = 0, 1, 2, 3, 4
CV_NS_BAD_KEY, CV_NS_SIGNATURES_MISSING, CV_NS_MALFORMED, CV_NS_CONFLICT = 5, 6, 7, 8
# cv_tearoff_sign_batch outcome[t] (CV_TS_*), its leaf_pre codes and first_bad's "no leaf"
CV_TS_SUCCESS, CV_TS_NO_LEAVES, CV_TS_MALFORMED, CV_TS_VERIFY_FAILED = 0, 1, 2, 3
CV_TS_NOT_COMMANDS, CV_TS_WRONG_COMMAND, CV_TS_UNKNOWN = 4, 5, 6
# cv_resolve_batch outcome[t] (CV_RS_*), graph[CV_RG_STATUS] (CV_RG_*) and the words of graph (RG_*)
CV_RS_OK, CV_RS_EMPTY, CV_RS_ID_MISMATCH, CV_RS_TX_INVALID, CV_RS_BAD_KEY = 0, 1, 2, 4, 5
CV_RS_SIGNATURES_MISSING, CV_RS_MALFORMED, CV_RS_BAD_INPUT, CV_RS_UNRESOLVED = 6, 7, 9, 10
CV_RG_OK, CV_RG_BAD_ID, CV_RG_DUPLICATE_ID = 0, 1, 2
RG_WORDS = ("status", "which", "n_pass", "stop_class", "stop_tx", "stop_input", "external", "maxprobe", "wraps")
RS_NONE = 0xFFFFFFFF              # input_dep: not in the batch; bad_input, graph: none
TS_PRE_OK, TS_PRE_NOT_COMMAND, TS_PRE_WRONG_COMMAND, TS_PRE_UNKNOWN = 0, 1, 2, 3
TS_NO_LEAF = 0xFFFFFFFF
NS_NO_SIG = 0xFFFFFFFF            # first_bad: no signature of the transaction settled its outcome
NS_PRE_SIGNATURE, NS_PRE_KEY = 1, 2   # sig_pre: the host prefilter's SignatureException / InvalidKeyException
CK_WIDE_DEFAULT, CK_WIDE_ALWAYS, CK_WIDE_NEVER = 0, 1, 0xFFFFFFFF      # cv_missing_signers' wide_min
CV_KS_ADDED = 0
CV_KS_PRESENT = 1
CV_KS_OK = 0
CV_KS_NO_KEY = 1
CV_ST_OK = 0
CV_ST_NO_KEY = 1
CV_ST_ALREADY_SIGNED = 2
CV_ST_EMPTY = 3
ST_NO_BAD = 0xFFFFFFFF            # first_bad of a CV_ST_OK transaction
CV_KS_STATS = ("resident", "capacity", "slots", "probe")   # CV_KS_STAT_*
CV_UNIQ_STATS = ("resident", "capacity", "slots", "rounds", "tail", "probe", "wraps")   # CV_UNIQ_STAT_*

# every symbol include/cordaverify.h declares (tests check the library exports all of them)
EXPORTED = (
    "cv_open", "cv_close", "cv_strerror", "cv_version", "cv_device_count",
    "cv_ed25519_verify_batch", "cv_merkle_tx_ids", "cv_merkle_tx_ids_ex", "cv_ed25519_sign_batch",
    "cv_tx_verdicts", "cv_ed25519_verify_device", "cv_ed25519_verify_device_timed", "cv_ed25519_sign_device", "cv_merkle_tx_ids_device",
    "cv_synchronize", "cv_calibrate", "cv_ed25519_verify_batch_keyed", "cv_key_cache_reserve", "cv_key_cache_stats",
    "cv_ed25519_verify_device_keyed", "cv_partial_merkle_verify", "cv_calibrate_cycles",
    "cv_diag_dedupe_keys", "cv_host_alloc", "cv_host_free", "cv_ed25519_verify_batch_async", "cv_wait",
    "cv_merkle_tx_ids_async", "cv_set_option", "cv_get_option", "cv_diag_stats",
    "cv_verify_transactions", "cv_verify_transactions_async", "cv_open_ex", "cv_msg_extent",
    "cv_ed25519_verify_batch_ex", "cv_merkle_tx_ids_bounded", "cv_verify_transactions_ex",
    "cv_signer_open", "cv_signer_public_key", "cv_signer_close", "cv_ed25519_sign_keyed",
    "cv_ed25519_sign_keyed_device", "cv_partial_merkle_build_bound", "cv_partial_merkle_build", "cv_filtered_build",
    "cv_uniq_open", "cv_uniq_close", "cv_uniq_reserve", "cv_uniq_commit_batch", "cv_uniq_lookup", "cv_uniq_load",
    "cv_uniq_set_max_rounds", "cv_uniq_stats", "cv_uniq_snapshot", "cv_uniq_clear", "cv_uniq_install",
    "cv_missing_signers", "cv_missing_signers_workspace", "cv_missing_signers_device",
    "cv_notarise_batch", "cv_filtered_verify", "cv_tearoff_sign_batch", "cv_resolve_batch",
    "cv_ed25519_dedupe_keys_device", "cv_ed25519_dedupe_keys_workspace",
    "cv_ed25519_verify_device_hotkeys", "cv_ed25519_verify_hotkeys_workspace",
    "cv_keystore_open", "cv_keystore_close", "cv_keystore_reserve", "cv_keystore_add", "cv_keystore_contains",
    "cv_keystore_sign", "cv_keystore_stats", "cv_sign_transactions",
)

# cv_set_option names (include/cordaverify.h CV_OPT_*)
OPTIONS = {"tri_max": 1, "quad_max": 2, "drain_split": 3, "drain_split_pct": 4, "pipe_min": 5, "pipe_first": 6,
           "pipe_chunk": 7, "async_chunk": 8, "host_threads": 9, "small_zero_copy": 10, "small_direct_min": 11,
           "auto_keyed": 12, "shard_min": 13, "spread_min": 14, "merkle_chunk": 15,
           "prep_overlap_min": 16, "timeline": 17, "pipe_split": 18,
           "pipe_overlap_first": 19, "mid_pieces": 20,
           "pipe_slots": 21, "txs_merkle_stream": 22, "fused_keyed": 23}
STATS = {"pipe": (0, ("plan_s", "pack_s", "wait_s", "enqueue_s", "sync_s", "calls", "subchunks", "direct_subchunks")),
         "small": (1, ("setup_s", "pack_s", "launch_s", "sync_s", "assemble_s", "calls")),
         "route": (2, ("calls", "routed_whole", "split_calls", "shards", "keyed_shards", "keyed_subchunks",
                       "merkle_calls", "merkle_subchunks")),
         "timeline": (3, ("ramp_ms", "dma_end_ms", "span_ms", "busy_ms", "idle_ms", "tail_ms", "result_copy_ms",
                          "first_subchunk", "merkle_busy_ms", "verify_busy_ms", "merkle_dma_end_ms", "groups",
                          "host_pre_ms", "host_post_ms", "calls")),
         "resolve": (4, ("upload_ms", "merkle_ms", "join_ms", "verify_ms", "signers_ms", "gate_ms", "readback_ms",
                         "host_order_ms", "calls"))}


class NativeUnavailable(RuntimeError):
    pass


class CvError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what}: {_lib.cv_strerror(code).decode() if _lib else code} (code {code})")
        self.code = code


_lib = None
_lock = threading.Lock()

_vp = ctypes.c_void_p
_sz = ctypes.c_size_t


def load():
    """Load the shared library (does not touch the GPU)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeUnavailable(f"{LIB_PATH} is missing: build it with `python -m corda_amd.build`")
        lib = ctypes.CDLL(LIB_PATH)
        lib.cv_open.argtypes = [ctypes.c_uint32, ctypes.POINTER(_vp)]
        lib.cv_open.restype = ctypes.c_int
        lib.cv_close.argtypes = [_vp]
        lib.cv_close.restype = None
        lib.cv_strerror.argtypes = [ctypes.c_int]
        lib.cv_strerror.restype = ctypes.c_char_p
        lib.cv_version.argtypes = []
        lib.cv_version.restype = ctypes.c_char_p
        lib.cv_device_count.argtypes = [_vp]
        lib.cv_device_count.restype = ctypes.c_int
        lib.cv_ed25519_verify_batch.argtypes = [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.cv_ed25519_verify_batch.restype = ctypes.c_int
        lib.cv_merkle_tx_ids.argtypes = [_vp, _sz, _vp, _vp, _vp, _vp, _vp]
        lib.cv_merkle_tx_ids.restype = ctypes.c_int
        lib.cv_merkle_tx_ids_ex.argtypes = [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.cv_merkle_tx_ids_async.argtypes = [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint64)]
        lib.cv_merkle_tx_ids_async.restype = ctypes.c_int
        lib.cv_verify_transactions.argtypes = [_vp, _sz] + [_vp] * 11
        lib.cv_verify_transactions.restype = ctypes.c_int
        lib.cv_verify_transactions_async.argtypes = [_vp, _sz] + [_vp] * 11 + [ctypes.POINTER(ctypes.c_uint64)]
        lib.cv_verify_transactions_ex.argtypes = [_vp, _sz, _vp, ctypes.c_uint64] + [_vp] * 10 + \
            [ctypes.POINTER(ctypes.c_uint64)]
        lib.cv_verify_transactions_ex.restype = ctypes.c_int
        lib.cv_merkle_tx_ids_bounded.argtypes = [_vp, _sz, _vp, ctypes.c_uint64] + [_vp] * 5 + \
            [ctypes.POINTER(ctypes.c_uint64)]
        lib.cv_merkle_tx_ids_bounded.restype = ctypes.c_int
        lib.cv_verify_transactions_async.restype = ctypes.c_int
        lib.cv_set_option.argtypes = [_vp, ctypes.c_int, ctypes.c_int64]
        lib.cv_set_option.restype = ctypes.c_int
        lib.cv_get_option.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
        lib.cv_get_option.restype = ctypes.c_int
        lib.cv_diag_stats.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), _sz, ctypes.c_int]
        lib.cv_diag_stats.restype = ctypes.c_int
        lib.cv_open_ex.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(_vp)]
        lib.cv_open_ex.restype = ctypes.c_int
        lib.cv_partial_merkle_verify.argtypes = [_vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]
        lib.cv_partial_merkle_verify.restype = ctypes.c_int
        lib.cv_merkle_tx_ids_ex.restype = ctypes.c_int
        lib.cv_partial_merkle_build_bound.argtypes = [_sz, _vp]
        lib.cv_partial_merkle_build_bound.restype = ctypes.c_uint64
        lib.cv_partial_merkle_build.argtypes = [_vp, _sz, _vp, _vp, _vp, _vp, _sz] + [_vp] * 7 + [ctypes.POINTER(_sz)]
        lib.cv_partial_merkle_build.restype = ctypes.c_int
        lib.cv_filtered_build.argtypes = [_vp, _sz, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, _sz] + [_vp] * 7 + \
            [ctypes.POINTER(_sz)]
        lib.cv_filtered_build.restype = ctypes.c_int
        lib.cv_ed25519_sign_batch.argtypes = [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.cv_ed25519_sign_batch.restype = ctypes.c_int
        lib.cv_ed25519_verify_batch_async.argtypes = [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                      ctypes.POINTER(ctypes.c_uint64)]
        lib.cv_ed25519_verify_batch_async.restype = ctypes.c_int
        lib.cv_ed25519_verify_batch_ex.argtypes = [_vp, _sz, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp,
                                                   ctypes.POINTER(ctypes.c_uint64)]
        lib.cv_ed25519_verify_batch_ex.restype = ctypes.c_int
        lib.cv_wait.argtypes = [_vp, ctypes.c_uint64]
        lib.cv_wait.restype = ctypes.c_int
        lib.cv_host_alloc.argtypes = [_vp, _sz, ctypes.POINTER(_vp)]
        lib.cv_host_alloc.restype = ctypes.c_int
        lib.cv_host_free.argtypes = [_vp, _vp]
        lib.cv_host_free.restype = None
        lib.cv_msg_extent.argtypes = [_sz, _vp, _vp]
        lib.cv_msg_extent.restype = ctypes.c_uint64
        lib.cv_tx_verdicts.argtypes = [_sz, _vp, _vp, _vp]
        lib.cv_tx_verdicts.restype = ctypes.c_int
        lib.cv_ed25519_verify_device.argtypes = [_vp, ctypes.c_int, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.cv_ed25519_verify_device.restype = ctypes.c_int
        lib.cv_ed25519_verify_device_timed.argtypes = [_vp, ctypes.c_int, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                       ctypes.POINTER(ctypes.c_float)]
        lib.cv_ed25519_verify_device_timed.restype = ctypes.c_int
        lib.cv_ed25519_sign_device.argtypes = [_vp, ctypes.c_int, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.cv_ed25519_sign_device.restype = ctypes.c_int
        lib.cv_signer_open.argtypes = [_vp, _vp, ctypes.POINTER(_vp)]
        lib.cv_signer_open.restype = ctypes.c_int
        lib.cv_signer_public_key.argtypes = [_vp, _vp]
        lib.cv_signer_public_key.restype = ctypes.c_int
        lib.cv_signer_close.argtypes = [_vp]
        lib.cv_signer_close.restype = None
        lib.cv_uniq_open.argtypes = [_vp, ctypes.c_int, _sz, ctypes.POINTER(_vp)]
        lib.cv_uniq_open.restype = ctypes.c_int
        lib.cv_uniq_close.argtypes = [_vp]
        lib.cv_uniq_close.restype = None
        lib.cv_uniq_reserve.argtypes = [_vp, _sz]
        lib.cv_uniq_reserve.restype = ctypes.c_int
        lib.cv_uniq_commit_batch.argtypes = [_vp, _sz] + [_vp] * 10
        lib.cv_uniq_commit_batch.restype = ctypes.c_int
        lib.cv_uniq_lookup.argtypes = [_vp, _sz] + [_vp] * 5
        lib.cv_uniq_lookup.restype = ctypes.c_int
        lib.cv_uniq_load.argtypes = [_vp, _sz] + [_vp] * 4
        lib.cv_uniq_load.restype = ctypes.c_int
        lib.cv_uniq_snapshot.argtypes = [_vp, _vp, _sz] + [_vp] * 5
        lib.cv_uniq_snapshot.restype = ctypes.c_int
        lib.cv_uniq_clear.argtypes = [_vp]
        lib.cv_uniq_clear.restype = ctypes.c_int
        lib.cv_uniq_install.argtypes = [_vp, _sz] + [_vp] * 4
        lib.cv_uniq_install.restype = ctypes.c_int
        lib.cv_uniq_set_max_rounds.argtypes = [_vp, ctypes.c_int]
        lib.cv_uniq_set_max_rounds.restype = ctypes.c_int
        lib.cv_uniq_stats.argtypes = [_vp, _vp, _sz]
        lib.cv_uniq_stats.restype = ctypes.c_int
        lib.cv_missing_signers.argtypes = [_vp] + [_sz] * 5 + [_vp] * 12 + [ctypes.c_uint32, _vp, _vp]
        lib.cv_missing_signers.restype = ctypes.c_int
        lib.cv_missing_signers_workspace.argtypes = [_sz, _sz]
        lib.cv_missing_signers_workspace.restype = ctypes.c_uint64
        lib.cv_missing_signers_device.argtypes = [_vp, ctypes.c_int] + [_sz] * 5 + [_vp] * 12 + [ctypes.c_uint32] + [_vp] * 4
        lib.cv_missing_signers_device.restype = ctypes.c_int
        lib.cv_notarise_batch.argtypes = ([_vp, _vp, _vp, ctypes.c_int, _sz, _vp, ctypes.c_uint64] + [_vp] * 11 + [_sz] * 3 +
                                          [_vp] * 19)
        lib.cv_notarise_batch.restype = ctypes.c_int
        lib.cv_filtered_verify.argtypes = [_vp, _sz, _vp, ctypes.c_uint64, _vp, _vp, _vp, _sz] + [_vp] * 8
        lib.cv_filtered_verify.restype = ctypes.c_int
        lib.cv_tearoff_sign_batch.argtypes = [_vp, _vp, _sz, _vp, ctypes.c_uint64, _vp, _vp, _vp, _sz] + [_vp] * 10
        lib.cv_tearoff_sign_batch.restype = ctypes.c_int
        lib.cv_resolve_batch.argtypes = ([_vp, _sz, _vp, ctypes.c_uint64] + [_vp] * 8 + [_sz] * 3 + [_vp] * 9 + [_sz] +
                                         [_vp] * 4 + [ctypes.c_uint64] + [_vp] * 9)
        lib.cv_resolve_batch.restype = ctypes.c_int
        lib.cv_ed25519_sign_keyed.argtypes = [_vp, _vp, _sz, _vp, ctypes.c_uint64, _vp, _vp, _vp]
        lib.cv_ed25519_sign_keyed.restype = ctypes.c_int
        lib.cv_ed25519_sign_keyed_device.argtypes = [_vp, ctypes.c_int, _vp, _sz, _vp, _vp, _vp, _vp, _vp]
        lib.cv_ed25519_sign_keyed_device.restype = ctypes.c_int
        lib.cv_merkle_tx_ids_device.argtypes = [_vp, ctypes.c_int, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.cv_merkle_tx_ids_device.restype = ctypes.c_int
        lib.cv_synchronize.argtypes = [_vp, ctypes.c_int]
        lib.cv_synchronize.restype = ctypes.c_int
        lib.cv_ed25519_verify_batch_keyed.argtypes = [_vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.cv_ed25519_verify_batch_keyed.restype = ctypes.c_int
        lib.cv_key_cache_reserve.argtypes = [_vp, _sz]
        lib.cv_key_cache_reserve.restype = ctypes.c_int
        lib.cv_key_cache_stats.argtypes = [_vp, ctypes.c_int, _vp]
        lib.cv_key_cache_stats.restype = ctypes.c_int
        lib.cv_ed25519_verify_device_keyed.argtypes = [_vp, ctypes.c_int, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp,
                                                       _vp, _vp, _vp, ctypes.POINTER(ctypes.c_float)]
        lib.cv_ed25519_verify_device_keyed.restype = ctypes.c_int
        if hasattr(lib, "cv_ed25519_dedupe_keys_device"):      # CV_LIB_PATH may name an older build (A/B tooling)
            lib.cv_ed25519_dedupe_keys_device.argtypes = [_vp, ctypes.c_int, _sz] + [_vp] * 6
            lib.cv_ed25519_dedupe_keys_device.restype = ctypes.c_int
            lib.cv_ed25519_dedupe_keys_workspace.argtypes = [_sz]
            lib.cv_ed25519_dedupe_keys_workspace.restype = ctypes.c_uint64
        if hasattr(lib, "cv_ed25519_verify_device_hotkeys"):
            lib.cv_ed25519_verify_device_hotkeys.argtypes = [_vp, ctypes.c_int, _sz] + [_vp] * 7 + [ctypes.c_uint32, _vp, _vp,
                                                                                                  _vp]
            lib.cv_ed25519_verify_device_hotkeys.restype = ctypes.c_int
            lib.cv_ed25519_verify_hotkeys_workspace.argtypes = [_sz]
            lib.cv_ed25519_verify_hotkeys_workspace.restype = ctypes.c_uint64
        if hasattr(lib, "cv_keystore_open"):
            lib.cv_keystore_open.argtypes = [_vp, ctypes.c_int, _sz, ctypes.POINTER(_vp)]
            lib.cv_keystore_open.restype = ctypes.c_int
            lib.cv_keystore_close.argtypes = [_vp]
            lib.cv_keystore_close.restype = None
            lib.cv_keystore_reserve.argtypes = [_vp, _sz]
            lib.cv_keystore_reserve.restype = ctypes.c_int
            lib.cv_keystore_add.argtypes = [_vp, _sz, _vp, _vp, _vp]
            lib.cv_keystore_add.restype = ctypes.c_int
            lib.cv_keystore_contains.argtypes = [_vp, _sz, _vp, _vp]
            lib.cv_keystore_contains.restype = ctypes.c_int
            lib.cv_keystore_sign.argtypes = [_vp, _sz, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp]
            lib.cv_keystore_sign.restype = ctypes.c_int
            lib.cv_keystore_stats.argtypes = [_vp, _vp, _sz]
            lib.cv_keystore_stats.restype = ctypes.c_int
            lib.cv_sign_transactions.argtypes = [_vp, _vp, _sz, _vp, ctypes.c_uint64, _vp, _vp, _vp, _sz] + [_vp] * 6
            lib.cv_sign_transactions.restype = ctypes.c_int
        lib.cv_calibrate.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        lib.cv_calibrate.restype = ctypes.c_int
        lib.cv_calibrate_cycles.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        lib.cv_calibrate_cycles.restype = ctypes.c_int
        lib.cv_diag_dedupe_keys.argtypes = [_sz, _vp, _vp, ctypes.POINTER(_sz)]
        lib.cv_diag_dedupe_keys.restype = ctypes.c_int
        _lib = lib
        return lib


_C0 = ctypes.c_char * 0


def _p(a: Optional[np.ndarray]):
    """The array's data pointer as an int (c_void_p arguments).  Through the buffer protocol: ~0.4 us per
    pointer against ~3 us for ndarray.ctypes.data_as, which a notary-sized call pays seven times; arrays the
    buffer protocol refuses (read-only, non-contiguous) take the ctypes attribute."""
    if a is None:
        return None
    try:
        return ctypes.addressof(_C0.from_buffer(a))
    except (TypeError, ValueError, BufferError):
        return a.ctypes.data


def _u8(a, shape_last=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a


def _msg_end(lib, off: np.ndarray, ln: np.ndarray) -> int:
    """max(off + len) — the arena bytes the records reach (multi-threaded in the library for big n)."""
    return int(lib.cv_msg_extent(off.shape[0], _p(off), _p(ln)))


def _ids_out(ids, ntx: int) -> np.ndarray:
    """The caller's optional ids output (the library writes ntx * 32 bytes into it): a new array when None,
    else it must be a writable, C-contiguous uint8 array of shape (ntx, 32) — a short or strided buffer would
    be written past its end or into the wrong bytes."""
    if ids is None:
        return np.zeros((ntx, 32), np.uint8)
    if not isinstance(ids, np.ndarray) or ids.dtype != np.uint8 or ids.shape != (ntx, 32):
        raise ValueError(f"ids must be a uint8 array of shape ({ntx}, 32)")
    if not ids.flags.c_contiguous or not ids.flags.writeable:
        raise ValueError("ids must be C-contiguous and writable")
    return ids


def _check(rc: int, what: str):
    if rc != CV_OK:
        raise CvError(rc, what)


# ---------------------------------------------------------------- marshalling (numpy alone: no library, no engine)
def pack_blobs(blobs) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Blobs back to back in one arena -> (arena u8, offsets u64, lengths u32).  The arena ends in 16 zero bytes, so
    it is never empty."""
    n = len(blobs)
    lens = np.fromiter((len(b) for b in blobs), dtype=np.uint32, count=n)
    offs = np.zeros(n, np.uint64)
    if n > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(blobs) + b"\0" * 16, np.uint8), offs, lens


def _arr(a, dt, n, what, width=1, exact=True):
    """a flat, of dt, with n rows of width entries (exact=False: at least); never empty: `width` zeros stand for it."""
    a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
    if a.size != n * width if exact else a.size < n * width:
        raise ValueError(f"{what} must have {n * width} entries, not {a.size}")
    return a if a.size else np.zeros(width, dt)


def _sig_args(sigs, ntx: int):
    """sigs = (pk (nsig,32), sig (nsig,64), tx_sig_begin u32[ntx+1], sig_pre u8[nsig] or None) -> (the four as the
    library takes them, nsig)."""
    pk, sg, tsb, sig_pre = sigs
    tsb = _arr(tsb, np.uint32, ntx + 1, "tx_sig_begin")
    nsig = int(tsb[-1])
    return [_arr(pk, np.uint8, nsig, "pk", 32), _arr(sg, np.uint8, nsig, "sig", 64), tsb,
            None if sig_pre is None else _arr(sig_pre, np.uint8, nsig, "sig_pre")], nsig


def _req_args(reqs, ntx: int, nsig: int, allowed: bool):
    """reqs = (kind, leaf_key, threshold, child_begin, child, weight, req_begin, tx_req_begin, sig_key), with
    req_allowed or None behind them when `allowed` -> (the nine or ten as the library takes them, nreq, nnodes,
    nchild)."""
    kind, leaf_key, threshold, child_begin, child, weight, req_begin, tx_req_begin, sig_key = reqs[:9]
    tx_req_begin = _arr(tx_req_begin, np.uint32, ntx + 1, "tx_req_begin")
    req_begin = np.ascontiguousarray(req_begin, dtype=np.uint32).reshape(-1)
    child_begin = np.ascontiguousarray(child_begin, dtype=np.uint32).reshape(-1)
    nreq, nnodes = req_begin.size - 1, child_begin.size - 1
    child = np.ascontiguousarray(child, dtype=np.uint32).reshape(-1)
    nchild = child.size
    if nreq < 0 or nnodes < 0:
        raise ValueError("the begin arrays must have count + 1 entries")
    a = [_arr(kind, np.uint8, nnodes, "kind"), _arr(leaf_key, np.uint8, nnodes, "leaf_key", 32),
         _arr(threshold, np.int32, nnodes, "threshold"), child_begin, child if nchild else np.zeros(1, np.uint32),
         _arr(weight, np.int32, nchild, "weight"), req_begin, tx_req_begin, _arr(sig_key, np.uint8, nsig, "sig_key", 32)]
    if allowed:
        (req_allowed,) = reqs[9:]
        a.append(None if req_allowed is None else _arr(req_allowed, np.uint8, nreq, "req_allowed"))
    return a, nreq, nnodes, nchild


def _outputs(names, fresh, out) -> list:
    """The output arrays of a call in the order of names: the caller's from `out` (None: passed as NULL), else new
    zeros of fresh[name] = (shape, dtype)."""
    out = dict(out or {})
    return [out[k] if k in out else np.zeros(*fresh[k]) for k in names]


def _cut_outputs(names, arrays, rows: dict, default: int) -> dict:
    """The outputs by name, each cut to its rows (rows[name], else default); None stays None."""
    return {k: None if a is None else a[:rows.get(k, default)] for k, a in zip(names, arrays)}


class Engine:
    """One context over a set of GPUs (bit d of device_mask = HIP device d; 0 = all).

    Host-buffer methods mirror the JVM drop-in (synchronous unless *_async); *_device methods take device
    pointers (ints, e.g. torch.Tensor.data_ptr()) and an optional hipStream_t (int), and return
    immediately.  The context is thread-safe: calls from several Python threads run concurrently (ctypes
    releases the GIL) and the engine routes them over its devices.
    virtual_devices (cv_open_ex): each GPU of the mask appears that many times in this context (independent
    device slots: the multi-device routing on a one-GPU box).
    """

    def __init__(self, device_mask: int = 0, virtual_devices: int = 1):
        lib = load()
        h = _vp()
        if virtual_devices != 1:
            rc = lib.cv_open_ex(ctypes.c_uint32(device_mask), int(virtual_devices), ctypes.byref(h))
        else:
            rc = lib.cv_open(ctypes.c_uint32(device_mask), ctypes.byref(h))
        if rc != CV_OK:
            raise NativeUnavailable(f"cv_open failed: {lib.cv_strerror(rc).decode()} (code {rc})")
        self._lib = lib
        self._h = h
        self.mu = threading.Lock()
        self._inflight = {}
        self._signers = weakref.WeakSet()   # open Signer and UniquenessSet objects: closed before their context

    def close(self):
        if self._h:
            for s in list(self._signers):
                s.close()
            self._lib.cv_close(self._h)
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

    @property
    def device_count(self) -> int:
        return self._lib.cv_device_count(self._h)

    # ------------------------------------------------------------ host-buffer API
    def host_empty(self, shape, dtype=np.uint8) -> np.ndarray:
        """An uninitialised numpy array in pinned host memory (cv_host_alloc), freed with its last view.
        Host-buffer calls whose five input arrays are all pinned skip the engine's packing copy."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        nbytes = max(1, int(np.prod(shape)) * np.dtype(dtype).itemsize)
        ptr = _vp()
        _check(self._lib.cv_host_alloc(self._h, nbytes, ctypes.byref(ptr)), "cv_host_alloc")
        buf = (ctypes.c_uint8 * nbytes).from_address(ptr.value)
        weakref.finalize(buf, self._lib.cv_host_free, None, ctypes.c_void_p(ptr.value))
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def host_copy(self, a) -> np.ndarray:
        """A pinned copy of array a (host_empty + copy)."""
        a = np.ascontiguousarray(a)
        out = self.host_empty(a.shape, a.dtype)
        out[...] = a
        return out

    def verify_batch(self, pk, sig, arena, off, ln, want_status: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """pk (n,32) u8, sig (n,64) u8, arena u8, off u64[n], ln u32[n] -> (bitmap u64[ceil(n/64)], status u8[n])."""
        pk = _u8(pk)
        sig = _u8(sig)
        n = pk.shape[0]
        if pk.size != n * 32 or sig.size != n * 64:
            raise ValueError("pk must be (n,32) and sig (n,64)")
        arena = _u8(arena) if arena is not None and np.asarray(arena).size else np.zeros(16, np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(ln, dtype=np.uint32)
        if off.shape[0] != n or ln.shape[0] != n:
            raise ValueError("off/len must have n entries")
        bitmap = np.zeros((n + 63) // 64, np.uint64)
        status = np.zeros(n, np.uint8) if want_status else None
        # the arena bound is checked by the engine's own staging scan (cv_ed25519_verify_batch_ex)
        rc = self._lib.cv_ed25519_verify_batch_ex(self._h, n, _p(pk), _p(sig), _p(arena), arena.size, _p(off), _p(ln),
                                                  _p(bitmap), _p(status), None)
        if rc == -3 and n and _msg_end(self._lib, off, ln) > arena.size:
            raise ValueError("message range exceeds the arena")
        _check(rc, "cv_ed25519_verify_batch")
        return bitmap, status

    def verify_batch_async(self, pk, sig, arena, off, ln, want_status: bool = True) -> int:
        """cv_ed25519_verify_batch_async: enqueue and return a ticket; wait(ticket) -> (bitmap, status).
        The arrays are kept referenced here until the wait (the engine may DMA from them until then)."""
        pk = _u8(pk)
        sig = _u8(sig)
        n = pk.shape[0]
        if pk.size != n * 32 or sig.size != n * 64:
            raise ValueError("pk must be (n,32) and sig (n,64)")
        arena = _u8(arena) if arena is not None and np.asarray(arena).size else np.zeros(16, np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(ln, dtype=np.uint32)
        if off.shape[0] != n or ln.shape[0] != n:
            raise ValueError("off/len must have n entries")
        bitmap = np.zeros((n + 63) // 64, np.uint64)
        status = np.zeros(n, np.uint8) if want_status else None
        t = ctypes.c_uint64()
        rc = self._lib.cv_ed25519_verify_batch_ex(self._h, n, _p(pk), _p(sig), _p(arena), arena.size, _p(off), _p(ln),
                                                  _p(bitmap), _p(status), ctypes.byref(t))
        if rc == -3 and n and _msg_end(self._lib, off, ln) > arena.size:
            raise ValueError("message range exceeds the arena")
        _check(rc, "cv_ed25519_verify_batch_async")
        with self.mu:
            self._inflight[t.value] = (bitmap, status, (pk, sig, arena, off, ln))
        return t.value

    def wait(self, ticket: int):
        """cv_wait: the results of an async call — (bitmap, status) for a verify, (ids, status) for Merkle ids."""
        with self.mu:
            a, b, keep = self._inflight.get(ticket, (None, None, None))
        _check(self._lib.cv_wait(self._h, ctypes.c_uint64(ticket)), "cv_wait")
        with self.mu:
            self._inflight.pop(ticket, None)
        del keep
        return a, b

    def verify_batch_keyed(self, keys, key_index, sig, arena, off, ln, want_status: bool = True):
        """keys (nk,32) distinct keys, key_index u32[n] -> (bitmap, status) exactly as verify_batch."""
        keys = _u8(keys)
        nk = keys.shape[0]
        key_index = np.ascontiguousarray(key_index, dtype=np.uint32)
        sig = _u8(sig)
        n = key_index.shape[0]
        if keys.size != nk * 32 or sig.size != n * 64:
            raise ValueError("keys must be (nk,32) and sig (n,64)")
        if n and int(key_index.max()) >= nk:
            raise ValueError("key_index out of range")
        arena = _u8(arena) if arena is not None and np.asarray(arena).size else np.zeros(16, np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(ln, dtype=np.uint32)
        if n and _msg_end(self._lib, off, ln) > arena.size:
            raise ValueError("message range exceeds the arena")
        bitmap = np.zeros((n + 63) // 64, np.uint64)
        status = np.zeros(n, np.uint8) if want_status else None
        _check(self._lib.cv_ed25519_verify_batch_keyed(self._h, n, nk, _p(keys), _p(key_index), _p(sig), _p(arena),
                                                       _p(off), _p(ln), _p(bitmap), _p(status)),
               "cv_ed25519_verify_batch_keyed")
        return bitmap, status

    def key_cache_reserve(self, max_keys: int):
        _check(self._lib.cv_key_cache_reserve(self._h, max_keys), "cv_key_cache_reserve")

    def key_cache_stats(self, device: int = 0) -> dict:
        out = np.zeros(4, np.uint64)
        _check(self._lib.cv_key_cache_stats(self._h, device, _p(out)), "cv_key_cache_stats")
        return {"resident": int(out[0]), "capacity": int(out[1]), "hits": int(out[2]), "misses": int(out[3])}

    def sign_batch(self, seeds, arena, off, ln) -> Tuple[np.ndarray, np.ndarray]:
        seeds = _u8(seeds)
        n = seeds.shape[0]
        arena = _u8(arena) if arena is not None and np.asarray(arena).size else np.zeros(16, np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(ln, dtype=np.uint32)
        pk = np.zeros((n, 32), np.uint8)
        sig = np.zeros((n, 64), np.uint8)
        _check(self._lib.cv_ed25519_sign_batch(self._h, n, _p(seeds), _p(arena), _p(off), _p(ln), _p(pk),
                                               _p(sig)), "cv_ed25519_sign_batch")
        return pk, sig

    @staticmethod
    def _merkle_args(arena, leaf_off, leaf_len, tx_leaf_begin, scan: bool = False):
        """The leaf arrays as the library takes them.  scan: also check the leaves against the arena here (the
        bounded entry points check it in the engine's own staging scan; this is their error path)."""
        tx_leaf_begin = np.ascontiguousarray(tx_leaf_begin, dtype=np.uint32)
        ntx = tx_leaf_begin.shape[0] - 1
        arena = _u8(arena) if arena is not None and np.asarray(arena).size else np.zeros(16, np.uint8)
        leaf_off = np.ascontiguousarray(leaf_off, dtype=np.uint64)
        leaf_len = np.ascontiguousarray(leaf_len, dtype=np.uint32)
        if leaf_off.size == 0:
            leaf_off = np.zeros(1, np.uint64)
            leaf_len = np.zeros(1, np.uint32)
        if leaf_off.shape[0] != leaf_len.shape[0] or (ntx > 0 and int(tx_leaf_begin[-1]) > leaf_off.shape[0]):
            raise ValueError("tx_leaf_begin reaches past the leaf arrays")
        if scan and ntx > 0 and int(tx_leaf_begin[-1]) and _msg_end(load(), leaf_off[:int(tx_leaf_begin[-1])],
                                                                    leaf_len[:int(tx_leaf_begin[-1])]) > arena.size:
            raise ValueError("leaf range exceeds the arena")
        return ntx, arena, leaf_off, leaf_len, tx_leaf_begin

    def _bounded_rc(self, rc: int, what: str, leaves):
        """A bounded call's return code: CV_E_ARGS from leaves past the arena (or wrapping) as ValueError, as
        the binding raised it when it scanned the leaves itself; any other error as CvError."""
        if rc == -3:
            self._merkle_args(*leaves, scan=True)   # raises ValueError for leaves past the arena
        _check(rc, what)

    def merkle_tx_ids(self, arena, leaf_off, leaf_len, tx_leaf_begin, ids=None) -> Tuple[np.ndarray, np.ndarray]:
        """WireTransaction.id of every transaction -> (ids (ntx,32) u8, status u8[ntx]).  ids: an optional
        output array (e.g. pinned, host_empty), so the ids are DMAed straight into it."""
        ntx, arena, leaf_off, leaf_len, tx_leaf_begin = self._merkle_args(arena, leaf_off, leaf_len, tx_leaf_begin)
        ids = _ids_out(ids, max(ntx, 0))
        st = np.zeros(max(ntx, 0), np.uint8)
        # the leaf-arena bound is checked by the engine's staging scan (cv_merkle_tx_ids_bounded)
        rc = self._lib.cv_merkle_tx_ids_bounded(self._h, ntx, _p(arena), arena.size, _p(leaf_off), _p(leaf_len),
                                                _p(tx_leaf_begin), _p(ids), _p(st), None)
        self._bounded_rc(rc, "cv_merkle_tx_ids_bounded", (arena, leaf_off, leaf_len, tx_leaf_begin))
        return ids, st

    def merkle_tx_ids_async(self, arena, leaf_off, leaf_len, tx_leaf_begin, ids=None) -> int:
        """cv_merkle_tx_ids_async: enqueue and return a ticket; wait(ticket) -> (ids, status)."""
        ntx, arena, leaf_off, leaf_len, tx_leaf_begin = self._merkle_args(arena, leaf_off, leaf_len, tx_leaf_begin)
        ids = _ids_out(ids, max(ntx, 0))
        st = np.zeros(max(ntx, 0), np.uint8)
        t = ctypes.c_uint64()
        rc = self._lib.cv_merkle_tx_ids_bounded(self._h, ntx, _p(arena), arena.size, _p(leaf_off), _p(leaf_len),
                                                _p(tx_leaf_begin), _p(ids), _p(st), ctypes.byref(t))
        self._bounded_rc(rc, "cv_merkle_tx_ids_bounded", (arena, leaf_off, leaf_len, tx_leaf_begin))
        with self.mu:
            self._inflight[t.value] = (ids, st, (arena, leaf_off, leaf_len, tx_leaf_begin))
        return t.value

    def _tx_args(self, arena, leaf_off, leaf_len, tx_leaf_begin, pk, sig, tx_sig_begin, ids, want_status,
                 want_sig_status):
        ntx, arena, leaf_off, leaf_len, tx_leaf_begin = self._merkle_args(arena, leaf_off, leaf_len, tx_leaf_begin)
        tx_sig_begin = np.ascontiguousarray(tx_sig_begin, dtype=np.uint32)
        if tx_sig_begin.shape[0] != ntx + 1:
            raise ValueError("tx_sig_begin must have ntx + 1 entries")
        pk = _u8(pk)
        sig = _u8(sig)
        nsig = int(tx_sig_begin[-1]) if ntx > 0 else 0
        if pk.size < nsig * 32 or sig.size < nsig * 64:
            raise ValueError("tx_sig_begin reaches past pk / sig")
        if pk.size == 0:
            pk, sig = np.zeros(32, np.uint8), np.zeros(64, np.uint8)
        ntx = max(ntx, 0)
        ids = _ids_out(ids, ntx)
        st = np.zeros(ntx, np.uint8) if want_status else None
        sst = np.zeros(nsig, np.uint8) if want_sig_status else None
        ok = np.zeros(ntx, np.uint8)
        args = (ntx, _p(arena), arena.size, _p(leaf_off), _p(leaf_len), _p(tx_leaf_begin), _p(pk), _p(sig),
                _p(tx_sig_begin), _p(ids), _p(st), _p(sst), _p(ok))
        return args, (ok, ids, st, sst), (arena, leaf_off, leaf_len, tx_leaf_begin, pk, sig, tx_sig_begin)

    def verify_transactions(self, arena, leaf_off, leaf_len, tx_leaf_begin, pk, sig, tx_sig_begin, ids=None,
                            want_status: bool = True, want_sig_status: bool = False):
        """cv_verify_transactions (SignedTransaction.verifySignatures' id + signature checks for a batch) ->
        (tx_ok u8[ntx], ids (ntx,32) u8, tx_status u8[ntx] or None, sig_status u8[nsig] or None)."""
        args, out, keep = self._tx_args(arena, leaf_off, leaf_len, tx_leaf_begin, pk, sig, tx_sig_begin, ids,
                                        want_status, want_sig_status)
        rc = self._lib.cv_verify_transactions_ex(self._h, *args, None)
        self._bounded_rc(rc, "cv_verify_transactions_ex", keep[:4])
        return out

    def verify_transactions_async(self, arena, leaf_off, leaf_len, tx_leaf_begin, pk, sig, tx_sig_begin, ids=None,
                                  want_status: bool = True, want_sig_status: bool = False) -> int:
        """cv_verify_transactions_async: enqueue and return a ticket; wait(ticket) -> (tx_ok, (ids, tx_status,
        sig_status))."""
        args, out, keep = self._tx_args(arena, leaf_off, leaf_len, tx_leaf_begin, pk, sig, tx_sig_begin, ids,
                                        want_status, want_sig_status)
        t = ctypes.c_uint64()
        rc = self._lib.cv_verify_transactions_ex(self._h, *args, ctypes.byref(t))
        self._bounded_rc(rc, "cv_verify_transactions_ex", keep[:4])
        with self.mu:
            self._inflight[t.value] = (out[0], out[1:], keep)
        return t.value

    # ------------------------------------------------------------ options and diagnostics
    def set_option(self, name: str, value: int):
        _check(self._lib.cv_set_option(self._h, OPTIONS[name], int(value)), f"cv_set_option({name})")

    def get_option(self, name: str) -> int:
        v = ctypes.c_int64()
        _check(self._lib.cv_get_option(self._h, OPTIONS[name], ctypes.byref(v)), f"cv_get_option({name})")
        return v.value

    def has_option(self, name: str) -> bool:
        """Whether the loaded library knows the option (CV_LIB_PATH may name an older build)."""
        return self._lib.cv_get_option(self._h, OPTIONS[name], ctypes.byref(ctypes.c_int64())) == CV_OK

    def stats(self, kind: str, reset: bool = False) -> dict:
        which, names = STATS[kind]
        out = (ctypes.c_double * len(names))()
        rc = self._lib.cv_diag_stats(self._h, which, out, len(names), int(reset))
        if rc < 0:
            raise CvError(rc, "cv_diag_stats")
        return dict(zip(names, out))

    def partial_merkle_verify(self, kind, left, right, leaf_hash, tree_begin, root, check, check_begin
                              ) -> Tuple[np.ndarray, np.ndarray]:
        """Flat partial Merkle trees (include/cordaverify.h) -> (verdict[ntrees], status[ntrees])."""
        tree_begin = np.ascontiguousarray(tree_begin, dtype=np.uint32)
        check_begin = np.ascontiguousarray(check_begin, dtype=np.uint32)
        ntrees = tree_begin.shape[0] - 1
        nnodes = int(tree_begin[-1]) if ntrees > 0 else 0
        ncheck = int(check_begin[-1]) if ntrees > 0 else 0

        def pad(a, dt, shape):
            a = np.ascontiguousarray(a, dtype=dt)
            return a if a.size else np.zeros(shape, dt)
        kind = pad(kind, np.uint8, 1)
        left = pad(left, np.uint32, 1)
        right = pad(right, np.uint32, 1)
        leaf_hash = pad(leaf_hash, np.uint8, (1, 32))
        root = pad(root, np.uint8, (1, 32))
        check = pad(check, np.uint8, (1, 32))
        verdict = np.zeros(max(ntrees, 1), np.uint8)
        status = np.zeros(max(ntrees, 1), np.uint8)
        _check(self._lib.cv_partial_merkle_verify(self._h, ntrees, nnodes, _p(kind), _p(left), _p(right),
                                                  _p(leaf_hash), _p(tree_begin), _p(root), ncheck, _p(check),
                                                  _p(check_begin), _p(verdict), _p(status)),
               "cv_partial_merkle_verify")
        return verdict[:ntrees], status[:ntrees]

    def _build_out(self, ntx: int, tx_leaf_begin: np.ndarray, nodes_cap: Optional[int]):
        cap = partial_merkle_build_bound(tx_leaf_begin) if nodes_cap is None else int(nodes_cap)
        m = max(cap, 1)
        return cap, (np.zeros(m, np.uint8), np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros((m, 32), np.uint8),
                     np.zeros(ntx + 1, np.uint32), np.zeros((max(ntx, 1), 32), np.uint8), np.zeros(max(ntx, 1), np.uint8))

    @staticmethod
    def _build_result(rc: int, what: str, ntx: int, cap: int, out, nn: int):
        """The node arrays cut to the nodes written; CV_E_ARGS from a short nodes_cap as ValueError with the count."""
        kind, left, right, hashes, tb, ids, st = out
        if rc == -3 and nn > cap:
            raise ValueError(f"{what}: the batch needs {nn} nodes, nodes_cap is {cap}")
        _check(rc, what)
        return kind[:nn], left[:nn], right[:nn], hashes[:nn], tb, ids[:ntx], st[:ntx]

    def partial_merkle_build(self, leaf_hash, tx_leaf_begin, include, include_begin, nodes_cap: Optional[int] = None):
        """cv_partial_merkle_build: PartialMerkleTree.build for every transaction, leaf_hash (nleaves,32) u8 and
        include (ninclude,32) u8 cut by tx_leaf_begin / include_begin (ntx+1 each) -> (kind, left, right,
        node_hash (nnodes,32), tree_begin u32[ntx+1], ids (ntx,32), status u8[ntx]): the first five are
        partial_merkle_verify's inputs as they stand.  nodes_cap: the node arrays' capacity (default: the bound)."""
        tx_leaf_begin = np.ascontiguousarray(tx_leaf_begin, dtype=np.uint32)
        include_begin = np.ascontiguousarray(include_begin, dtype=np.uint32)
        ntx = tx_leaf_begin.shape[0] - 1
        if ntx < 0 or include_begin.shape[0] != ntx + 1:
            raise ValueError("tx_leaf_begin and include_begin must have ntx + 1 entries")
        leaf_hash = _u8(leaf_hash)
        include = _u8(include)
        if ntx and (leaf_hash.size < 32 * int(tx_leaf_begin[-1]) or include.size < 32 * int(include_begin[-1])):
            raise ValueError("the ranges reach past leaf_hash / include")
        if leaf_hash.size == 0:
            leaf_hash = np.zeros(32, np.uint8)
        if include.size == 0:
            include = np.zeros(32, np.uint8)
        cap, out = self._build_out(ntx, tx_leaf_begin, nodes_cap)
        nn = _sz(0)
        rc = self._lib.cv_partial_merkle_build(self._h, ntx, _p(leaf_hash), _p(tx_leaf_begin), _p(include),
                                               _p(include_begin), cap, *[_p(a) for a in out], ctypes.byref(nn))
        return self._build_result(rc, "cv_partial_merkle_build", ntx, cap, out, nn.value)

    def filtered_build(self, arena, leaf_off, leaf_len, tx_leaf_begin, keep, nodes_cap: Optional[int] = None):
        """cv_filtered_build: FilteredTransaction.buildMerkleTransaction's trees for every transaction, the leaf
        blobs as merkle_tx_ids takes them and keep u8[nleaves] (non-zero: the filters keep the leaf) -> as
        partial_merkle_build (ids = the transactions' ids)."""
        ntx, arena, leaf_off, leaf_len, tx_leaf_begin = self._merkle_args(arena, leaf_off, leaf_len, tx_leaf_begin)
        if ntx < 0:
            raise ValueError("tx_leaf_begin must have ntx + 1 entries")
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if ntx and keep.shape[0] < int(tx_leaf_begin[-1]):
            raise ValueError("keep must have one entry per leaf")
        if keep.size == 0:
            keep = np.zeros(1, np.uint8)
        cap, out = self._build_out(ntx, tx_leaf_begin, nodes_cap)
        nn = _sz(0)
        rc = self._lib.cv_filtered_build(self._h, ntx, _p(arena), arena.size, _p(leaf_off), _p(leaf_len),
                                         _p(tx_leaf_begin), _p(keep), cap, *[_p(a) for a in out], ctypes.byref(nn))
        # not _bounded_rc: here CV_E_ARGS also reports a nodes_cap that is too small, which _build_result words
        if rc == -3 and nn.value <= cap:
            self._merkle_args(arena, leaf_off, leaf_len, tx_leaf_begin, scan=True)   # leaves past the arena: ValueError
        return self._build_result(rc, "cv_filtered_build", ntx, cap, out, nn.value)

    def missing_signers(self, kind, leaf_key, threshold, child_begin, child, weight, req_begin, tx_req_begin, sig_key,
                        tx_sig_begin, req_allowed=None, bitmap=None, wide_min: int = CK_WIDE_DEFAULT
                        ) -> Tuple[np.ndarray, np.ndarray]:
        """cv_missing_signers: the flat CompositeKey encoding of include/cordaverify.h (transactions.flatten_must_sign
        builds it) -> (req_missing u8[nreq]: 0 fulfilled, 1 missing, 2 malformed; tx_status u8[ntx]: CV_VS_*).
        req_allowed u8[nreq] and bitmap u64[ceil(nsig / 64)] are optional; wide_min forces a path (CK_WIDE_*)."""
        tx_req_begin = np.ascontiguousarray(tx_req_begin, dtype=np.uint32).reshape(-1)
        tx_sig_begin = np.ascontiguousarray(tx_sig_begin, dtype=np.uint32).reshape(-1)
        ntx = tx_req_begin.size - 1
        if ntx < 0 or tx_sig_begin.size != ntx + 1:
            raise ValueError("the begin arrays must have count + 1 entries")
        sig_key = np.ascontiguousarray(sig_key, dtype=np.uint8).reshape(-1)
        if sig_key.size % 32:
            raise ValueError("sig_key must be rows of 32 bytes")
        nsig = sig_key.size // 32
        a_req, nreq, nnodes, nchild = _req_args((kind, leaf_key, threshold, child_begin, child, weight, req_begin,
                                                 tx_req_begin, sig_key, req_allowed), ntx, nsig, allowed=True)
        if bitmap is not None:
            bitmap = _arr(bitmap, np.uint64, (nsig + 63) // 64, "bitmap")
        req_missing = np.zeros(max(nreq, 1), np.uint8)
        tx_status = np.zeros(max(ntx, 1), np.uint8)
        _check(self._lib.cv_missing_signers(self._h, ntx, nreq, nnodes, nchild, nsig, *[_p(a) for a in a_req[:9]],
                                            _p(tx_sig_begin), _p(a_req[9]), _p(bitmap), ctypes.c_uint32(wide_min),
                                            _p(req_missing), _p(tx_status)),
               "cv_missing_signers")
        return req_missing[:nreq], tx_status[:ntx]

    NOTARISE_OUTPUTS = ("outcome", "ids", "notary_sig", "first_bad", "req_missing", "state_conflict", "consumed_id",
                        "consumed_index", "consumed_caller")

    def notarise_batch(self, uniq: "UniquenessSet", signer: "Signer", arena, leaf_off, leaf_len, tx_leaf_begin,
                       tx_input_count, claimed_id, caller, tx_pre=None, sigs=None, reqs=None, out=None) -> dict:
        """cv_notarise_batch: the notary's commit step for a batch in one call (ids, signatures, missing signers, the
        commit on `uniq`, the notary's signatures with `signer`).  Leaves as merkle_tx_ids; the states of transaction
        t are its first tx_input_count[t] leaves; claimed_id (ntx,32) u8; caller u32[ntx]; tx_pre u8[ntx] or None.
        sigs = (pk (nsig,32), sig (nsig,64), tx_sig_begin u32[ntx+1], sig_pre u8[nsig] or None) makes the call
        validating, with reqs = the arrays of missing_signers up to sig_key, then req_allowed or None: (kind, leaf_key,
        threshold, child_begin, child, weight, req_begin, tx_req_begin, sig_key, req_allowed).  sigs None: the simple
        notary.  Returns a dict of NOTARISE_OUTPUTS (include/cordaverify.h).  out: arrays to write into by name; an
        optional output given as None is passed as NULL and comes back None.  CvError -4 when the set would pass its
        capacity: nothing changed and nothing written."""
        ntx, arena, leaf_off, leaf_len, tx_leaf_begin = self._merkle_args(arena, leaf_off, leaf_len, tx_leaf_begin)
        tx_input_count = _arr(tx_input_count, np.uint32, ntx, "tx_input_count")
        claimed_id = _arr(claimed_id, np.uint8, ntx, "claimed_id", 32)
        caller = _arr(caller, np.uint32, ntx, "caller")
        if tx_pre is not None:
            tx_pre = _arr(tx_pre, np.uint8, ntx, "tx_pre")
        ns = int(tx_input_count[:ntx].sum())
        nreq = nnodes = nchild = 0
        a_sig = [None] * 4
        a_req = [None] * 10
        if sigs is not None:
            if reqs is None:
                raise ValueError("a validating call needs the requirement arrays")
            a_sig, nsig = _sig_args(sigs, ntx)
            a_req, nreq, nnodes, nchild = _req_args(reqs, ntx, nsig, allowed=True)
        m, q = max(ns, 1), max(ntx, 1)
        o = _outputs(self.NOTARISE_OUTPUTS,
                     {"outcome": (q, np.uint8), "ids": ((q, 32), np.uint8), "notary_sig": ((q, 64), np.uint8),
                      "first_bad": (q, np.uint32), "req_missing": (max(nreq, 1), np.uint8), "state_conflict": (m, np.uint8),
                      "consumed_id": ((m, 32), np.uint8), "consumed_index": (m, np.uint32),
                      "consumed_caller": (m, np.uint32)}, out)
        rc = self._lib.cv_notarise_batch(self._h, uniq._open(), signer._h, 1 if sigs is not None else 0, ntx, _p(arena),
                                         arena.size, _p(leaf_off), _p(leaf_len), _p(tx_leaf_begin), _p(tx_input_count),
                                         _p(claimed_id), _p(caller), _p(tx_pre), *[_p(a) for a in a_sig], nreq, nnodes,
                                         nchild, *[_p(a) for a in a_req], *[_p(a) for a in o])
        self._bounded_rc(rc, "cv_notarise_batch", (arena, leaf_off, leaf_len, tx_leaf_begin))
        return _cut_outputs(self.NOTARISE_OUTPUTS, o,
                            {"outcome": ntx, "ids": ntx, "notary_sig": ntx, "first_bad": ntx, "req_missing": nreq}, ns)

    def _tearoff_args(self, arena, leaf_off, leaf_len, tx_leaf_begin, kind, left, right, node_hash, tree_begin, root):
        """The shared inputs of filtered_verify and tearoff_sign_batch as the library takes them."""
        ntx, arena, leaf_off, leaf_len, tx_leaf_begin = self._merkle_args(arena, leaf_off, leaf_len, tx_leaf_begin)
        tree_begin = np.ascontiguousarray(tree_begin, dtype=np.uint32)
        if ntx < 0 or tree_begin.shape[0] != ntx + 1:
            raise ValueError("tx_leaf_begin and tree_begin must have ntx + 1 entries")
        nnodes = int(tree_begin[-1]) if ntx else 0
        # exact=False: longer arrays pass, the ranges say what is read
        nodes = [_arr(kind, np.uint8, nnodes, "kind", exact=False), _arr(left, np.uint32, nnodes, "left", exact=False),
                 _arr(right, np.uint32, nnodes, "right", exact=False),
                 _arr(node_hash, np.uint8, nnodes, "node_hash", 32, exact=False)]
        root = _arr(root, np.uint8, ntx, "root", 32, exact=False)
        return ntx, nnodes, (arena, leaf_off, leaf_len, tx_leaf_begin), nodes, tree_begin, root

    def filtered_verify(self, arena, leaf_off, leaf_len, tx_leaf_begin, kind, left, right, node_hash, tree_begin, root
                        ) -> Tuple[np.ndarray, np.ndarray]:
        """cv_filtered_verify: FilteredTransaction.verify for every tear-off from its FILTERED leaves' blobs (as
        merkle_tx_ids takes them, cut by tx_leaf_begin) and the flat trees of partial_merkle_verify / filtered_build
        -> (verdict[ntx], status[ntx]); status CV_PMT_NO_INCLUDED for a tear-off without filtered leaves."""
        ntx, nnodes, (arena, leaf_off, leaf_len, txb), nodes, tree_begin, root = self._tearoff_args(
            arena, leaf_off, leaf_len, tx_leaf_begin, kind, left, right, node_hash, tree_begin, root)
        verdict, status = np.zeros(max(ntx, 1), np.uint8), np.zeros(max(ntx, 1), np.uint8)
        rc = self._lib.cv_filtered_verify(self._h, ntx, _p(arena), arena.size, _p(leaf_off), _p(leaf_len), _p(txb), nnodes,
                                          *[_p(a) for a in nodes], _p(tree_begin), _p(root), _p(verdict), _p(status))
        self._bounded_rc(rc, "cv_filtered_verify", (arena, leaf_off, leaf_len, txb))
        return verdict[:ntx], status[:ntx]

    def tearoff_sign_batch(self, signer: "Signer", arena, leaf_off, leaf_len, tx_leaf_begin, kind, left, right, node_hash,
                           tree_begin, root, leaf_pre=None, out=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """cv_tearoff_sign_batch: NodeInterestRates.Oracle.sign for every tear-off in one call — the inputs of
        filtered_verify, leaf_pre u8[nleaves] or None (TS_PRE_*: the service's verdict on each filtered leaf) ->
        (outcome u8[ntx] CV_TS_*, first_bad u32[ntx], sig (ntx,64) u8: the signer's signature over the root of an
        accepted tear-off, zero bytes for a refused one).  out: (outcome, first_bad or None, sig) to write into."""
        ntx, nnodes, (arena, leaf_off, leaf_len, txb), nodes, tree_begin, root = self._tearoff_args(
            arena, leaf_off, leaf_len, tx_leaf_begin, kind, left, right, node_hash, tree_begin, root)
        nl = int(txb[-1]) if ntx else 0
        if leaf_pre is not None:
            leaf_pre = np.ascontiguousarray(leaf_pre, dtype=np.uint8).reshape(-1)
            if leaf_pre.size < nl:
                raise ValueError("leaf_pre must have one entry per filtered leaf")
            if leaf_pre.size == 0:
                leaf_pre = np.zeros(1, np.uint8)
        q = max(ntx, 1)
        outcome, first_bad, sig = out if out is not None else (np.zeros(q, np.uint8), np.zeros(q, np.uint32),
                                                               np.zeros((q, 64), np.uint8))
        if not signer._h:
            raise ValueError("the signer is closed")
        rc = self._lib.cv_tearoff_sign_batch(self._h, signer._h, ntx, _p(arena), arena.size, _p(leaf_off), _p(leaf_len),
                                             _p(txb), nnodes, *[_p(a) for a in nodes], _p(tree_begin), _p(root),
                                             _p(leaf_pre), _p(outcome), _p(first_bad), _p(sig))
        self._bounded_rc(rc, "cv_tearoff_sign_batch", (arena, leaf_off, leaf_len, txb))
        return outcome[:ntx], None if first_bad is None else first_bad[:ntx], sig[:ntx]

    RESOLVE_OUTPUTS = ("outcome", "first_bad", "req_missing", "bad_input", "input_dep", "input_status", "order", "graph",
                       "ids")

    def resolve_batch(self, arena, leaf_off, leaf_len, tx_leaf_begin, claimed_id, sigs, reqs, tx_input_begin,
                      input_txhash, input_index, tx_output_count, seed: int = 0, out=None) -> dict:
        """cv_resolve_batch: ResolveTransactionsFlow.call over the downloaded transactions, in download order, in one
        call (ids, signatures, missing signers, the join of every input against the batch, the duplicate check,
        topologicalSort and the walk to its first failure).  Leaves as merkle_tx_ids; claimed_id (ntx,32) u8;
        sigs = (pk (nsig,32), sig (nsig,64), tx_sig_begin u32[ntx+1], sig_pre u8[nsig] or None); reqs = the arrays of
        missing_signers up to sig_key: (kind, leaf_key, threshold, child_begin, child, weight, req_begin, tx_req_begin,
        sig_key); the graph: tx_input_begin u32[ntx+1], input_txhash (ninputs,32) u8, input_index u32[ninputs],
        tx_output_count u32[ntx]; seed 0 draws a fresh one.  Returns a dict of RESOLVE_OUTPUTS
        (include/cordaverify.h; graph u32[9], see RG_WORDS).  out: arrays to write into by name; an optional output
        (first_bad, req_missing, ids) given as None is passed as NULL and comes back None."""
        ntx, arena, leaf_off, leaf_len, tx_leaf_begin = self._merkle_args(arena, leaf_off, leaf_len, tx_leaf_begin)
        if ntx < 0:
            raise ValueError("tx_leaf_begin must have ntx + 1 entries")
        claimed_id = _arr(claimed_id, np.uint8, ntx, "claimed_id", 32)
        a_sig, nsig = _sig_args(sigs, ntx)
        a_req, nreq, nnodes, nchild = _req_args(reqs, ntx, nsig, allowed=False)
        tib = _arr(tx_input_begin, np.uint32, ntx + 1, "tx_input_begin")
        nin = int(tib[-1])
        a_graph = [tib, _arr(input_txhash, np.uint8, nin, "input_txhash", 32),
                   _arr(input_index, np.uint32, nin, "input_index"), _arr(tx_output_count, np.uint32, ntx, "tx_output_count")]
        m, q = max(nin, 1), max(ntx, 1)
        o = _outputs(self.RESOLVE_OUTPUTS,
                     {"outcome": (q, np.uint8), "first_bad": (q, np.uint32), "req_missing": (max(nreq, 1), np.uint8),
                      "bad_input": (q, np.uint32), "input_dep": (m, np.uint32), "input_status": (m, np.uint8),
                      "order": (q, np.uint32), "graph": (len(RG_WORDS), np.uint32), "ids": ((q, 32), np.uint8)}, out)
        rc = self._lib.cv_resolve_batch(self._h, ntx, _p(arena), arena.size, _p(leaf_off), _p(leaf_len), _p(tx_leaf_begin),
                                        _p(claimed_id), *[_p(a) for a in a_sig], nreq, nnodes, nchild,
                                        *[_p(a) for a in a_req], nin, *[_p(a) for a in a_graph], ctypes.c_uint64(seed),
                                        *[_p(a) for a in o])
        self._bounded_rc(rc, "cv_resolve_batch", (arena, leaf_off, leaf_len, tx_leaf_begin))
        return _cut_outputs(self.RESOLVE_OUTPUTS, o, {"req_missing": nreq, "input_dep": nin, "input_status": nin,
                                                      "graph": len(RG_WORDS)}, ntx)

    # ------------------------------------------------------------ device-resident API
    def missing_signers_device(self, device: int, ntx: int, nreq: int, nnodes: int, nchild: int, nsig: int, d_kind: int,
                               d_leaf_key: int, d_threshold: int, d_child_begin: int, d_child: int, d_weight: int,
                               d_req_begin: int, d_tx_req_begin: int, d_sig_key: int, d_tx_sig_begin: int,
                               d_req_allowed: int, d_bitmap: int, wide_min: int, d_req_missing: int, d_tx_status: int,
                               d_workspace: int, stream: int = 0):
        """cv_missing_signers_device: enqueued on `stream`, nothing synchronised; d_workspace of
        missing_signers_workspace(ntx, nnodes) bytes.  d_req_allowed / d_bitmap 0: none allowed / all valid."""
        _check(self._lib.cv_missing_signers_device(
            self._h, device, ntx, nreq, nnodes, nchild, nsig, d_kind or None, d_leaf_key or None, d_threshold or None,
            d_child_begin or None, d_child or None, d_weight or None, d_req_begin or None, d_tx_req_begin or None,
            d_sig_key or None, d_tx_sig_begin or None, d_req_allowed or None, d_bitmap or None,
            ctypes.c_uint32(wide_min), d_req_missing or None, d_tx_status or None, d_workspace or None, stream or None),
            "cv_missing_signers_device")

    def verify_device(self, device: int, n: int, d_pk: int, d_sig: int, d_arena: int, d_off: int, d_len: int,
                      d_bitmap: int, d_status: int = 0, stream: int = 0):
        _check(self._lib.cv_ed25519_verify_device(self._h, device, n, d_pk, d_sig, d_arena, d_off, d_len, d_bitmap,
                                                  d_status or None, stream or None), "cv_ed25519_verify_device")

    def verify_device_timed(self, device: int, n: int, d_pk: int, d_sig: int, d_arena: int, d_off: int, d_len: int,
                            d_bitmap: int, stream: int = 0) -> Tuple[float, float, float]:
        """Synchronous verify; returns three kernel durations in ms (HIP events): (scalars, points,
        hs_straus) for throughput batches, (scalars + point pairs, 0, tri / quad Straus) for latency ones."""
        ms = (ctypes.c_float * 3)()
        _check(self._lib.cv_ed25519_verify_device_timed(self._h, device, n, d_pk, d_sig, d_arena, d_off, d_len,
                                                        d_bitmap, stream or None, ms), "cv_ed25519_verify_device_timed")
        return ms[0], ms[1], ms[2]

    def verify_device_keyed(self, device: int, n: int, nkeys: int, d_keys: int, d_key_index: int, d_sig: int,
                            d_arena: int, d_off: int, d_len: int, d_bitmap: int, d_status: int = 0, stream: int = 0,
                            timed: bool = False):
        """Keyed device batch; with timed=True synchronous, returns (keyprep, hash, comb, finish) ms."""
        ms = (ctypes.c_float * 4)() if timed else None
        _check(self._lib.cv_ed25519_verify_device_keyed(self._h, device, n, nkeys, d_keys, d_key_index, d_sig, d_arena,
                                                        d_off, d_len, d_bitmap, d_status or None, stream or None, ms),
               "cv_ed25519_verify_device_keyed")
        return tuple(ms) if timed else None

    def dedupe_keys_device(self, device: int, n: int, d_pk: int, d_keys: int, d_key_index: int, d_nkeys: int,
                           d_workspace: int, stream: int = 0):
        """The distinct keys of d_pk[n][32] on the device: d_keys (n * 32 bytes, the first nkeys rows written, first-seen
        order), d_key_index (n uint32), d_nkeys (one uint32); d_workspace of dedupe_keys_workspace(n) bytes.  Enqueues
        and returns; what verify_device_keyed takes."""
        _check(self._lib.cv_ed25519_dedupe_keys_device(self._h, device, n, d_pk or None, d_keys or None,
                                                       d_key_index or None, d_nkeys or None, d_workspace or None,
                                                       stream or None), "cv_ed25519_dedupe_keys_device")

    def verify_device_hotkeys(self, device: int, n: int, d_pk: int, d_sig: int, d_arena: int, d_off: int, d_len: int,
                              d_bitmap: int, d_status: int, d_workspace: int, hot_min: int = 0, stream: int = 0) -> dict:
        """The hot-key route over device arrays (cv_ed25519_verify_device_hotkeys): the records of keys that occur at
        least hot_min times (0: 8) through the keyed path, the rest through the unkeyed one; d_bitmap and d_status
        (0: none) as verify_device writes them.  d_workspace of verify_hotkeys_workspace(n) bytes.  Synchronises the
        stream once, enqueues the verifies and returns the split: nkeys, hot_keys, hot, cold."""
        route = (ctypes.c_uint32 * 4)()
        _check(self._lib.cv_ed25519_verify_device_hotkeys(self._h, device, n, d_pk or None, d_sig or None, d_arena or None,
                                                          d_off or None, d_len or None, d_bitmap or None, d_status or None,
                                                          hot_min, d_workspace or None, stream or None, route),
               "cv_ed25519_verify_device_hotkeys")
        return dict(nkeys=route[0], hot_keys=route[1], hot=route[2], cold=route[3])

    def sign_device(self, device: int, n: int, d_seed: int, d_arena: int, d_off: int, d_len: int, d_pk: int,
                    d_sig: int, stream: int = 0):
        _check(self._lib.cv_ed25519_sign_device(self._h, device, n, d_seed, d_arena, d_off, d_len, d_pk, d_sig,
                                                stream or None), "cv_ed25519_sign_device")

    def merkle_device(self, device: int, ntx: int, nleaves: int, d_arena: int, d_off: int, d_len: int,
                      d_tx_begin: int, d_workspace: int, d_ids: int, d_status: int = 0, stream: int = 0):
        _check(self._lib.cv_merkle_tx_ids_device(self._h, device, ntx, nleaves, d_arena, d_off, d_len, d_tx_begin,
                                                 d_workspace, d_ids, d_status or None, stream or None),
               "cv_merkle_tx_ids_device")

    def calibrate(self, device: int) -> Tuple[float, float]:
        """(v_mad_u64_u32 per second, fe_mul per second) measured on `device` (roofline peak)."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        _check(self._lib.cv_calibrate(self._h, device, ctypes.byref(a), ctypes.byref(b)), "cv_calibrate")
        return a.value, b.value

    def calibrate_cycles(self, device: int) -> dict:
        """The v_mad_u64_u32 peak on a cycle basis (cv_calibrate_cycles)."""
        o = (ctypes.c_double * 5)()
        _check(self._lib.cv_calibrate_cycles(self._h, device, o), "cv_calibrate_cycles")
        return {"mac_per_s": o[0], "clock_ghz": o[1], "cycles_per_wave_instr": o[2], "simds": int(o[3]),
                "mac_per_s_at_2p4ghz": o[4]}

    def synchronize(self, device: int):
        _check(self._lib.cv_synchronize(self._h, device), "cv_synchronize")


class _Handle:
    """The life of a native handle bound to an engine: close() once (and again without effect), the with-statement,
    the finaliser, and _open(), which hands the handle out or says that it is closed.  A subclass names its close
    entry point and itself, sets _engine, _lib and _h, and adds itself to engine._signers."""

    _close_fn = _what = None

    def close(self):
        if self._h:
            getattr(self._lib, self._close_fn)(self._h)
            self._h = None
            self._engine._signers.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self):
        if not self._h:
            raise ValueError(f"the {self._what} is closed")
        return self._h


class Signer(_Handle):
    """One Ed25519 key bound to an engine (cv_signer): the key is expanded once on every device, then
    sign() / sign_device() sign batches with it — KeyPair.signWithECDSA (CryptoUtilities.kt:63-73) for a
    holder of one long-lived key, such as a notary.  Immutable after construction: several threads may sign
    with it at once.  close() (or the with-statement) wipes the device records; the engine closes the
    signers still open when it is closed itself."""

    _close_fn, _what = "cv_signer_close", "signer"

    def __init__(self, engine: Engine, seed):
        seed = np.frombuffer(bytes(seed), np.uint8)
        if seed.size != 32:
            raise ValueError("seed must be 32 bytes")
        self._engine = engine
        self._lib = engine._lib
        h = _vp()
        _check(self._lib.cv_signer_open(engine._h, _p(seed), ctypes.byref(h)), "cv_signer_open")
        self._h = h
        pk = np.zeros(32, np.uint8)
        _check(self._lib.cv_signer_public_key(h, _p(pk)), "cv_signer_public_key")
        self.public_key = pk.tobytes()
        engine._signers.add(self)

    def sign(self, arena, off, ln) -> np.ndarray:
        """arena u8, off u64[n], ln u32[n] -> sig (n,64) u8, one signature per message, in one call."""
        self._open()
        arena = _u8(arena) if arena is not None and np.asarray(arena).size else np.zeros(16, np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(ln, dtype=np.uint32)
        n = off.shape[0]
        if ln.shape[0] != n:
            raise ValueError("off/len must have n entries")
        sig = np.zeros((n, 64), np.uint8)
        rc = self._lib.cv_ed25519_sign_keyed(self._engine._h, self._h, n, _p(arena), arena.size, _p(off), _p(ln),
                                             _p(sig))
        if rc == -3 and n and _msg_end(self._lib, off, ln) > arena.size:
            raise ValueError("message range exceeds the arena")
        _check(rc, "cv_ed25519_sign_keyed")
        return sig

    def sign_device(self, device: int, n: int, d_arena: int, d_off: int, d_len: int, d_sig: int, stream: int = 0):
        """Device pointers in, d_sig[n][64] out; enqueued on stream (0: the device's own), not synchronised."""
        self._open()
        _check(self._lib.cv_ed25519_sign_keyed_device(self._engine._h, device, self._h, n, d_arena, d_off, d_len,
                                                      d_sig, stream or None), "cv_ed25519_sign_keyed_device")


class KeyStore(_Handle):
    """A device-resident store of expanded private keys addressed by public key, bound to an engine (cv_keystore): the
    node's KeyManagementService (Services.kt:206-219, PersistentKeyManagementService.kt:40-66) — add() is freshKey() for
    a batch of seeds, contains() is keys.contains, sign() is KeyPair(pk, toPrivate(pk)).signWithECDSA with every record
    naming its own key, sign_transactions() the builder's signing step (TransactionBuilder.kt:93-98,132-141) for a
    batch.  No call gives out a private half.  Calls serialise on the store's own lock.  close() (or the
    with-statement) overwrites and frees the table; the engine closes the stores still open when it is closed itself."""

    _close_fn, _what = "cv_keystore_close", "key store"

    def __init__(self, engine: Engine, capacity: int, device: int = 0):
        self._engine = engine
        self._lib = engine._lib
        h = _vp()
        _check(self._lib.cv_keystore_open(engine._h, device, int(capacity), ctypes.byref(h)), "cv_keystore_open")
        self._h = h
        engine._signers.add(self)

    def add(self, seeds):
        """cv_keystore_add: seeds (n,32) u8 -> (pk (n,32) u8, status u8[n]: CV_KS_ADDED | CV_KS_PRESENT).  CvError with
        code -4 when resident + n would pass the capacity: nothing changed, reserve() first."""
        h = self._open()
        seeds = _u8(seeds).reshape(-1)
        if seeds.size % 32:
            raise ValueError("seeds must be n x 32 bytes")
        n = seeds.size // 32
        pk, st = np.zeros((max(n, 1), 32), np.uint8), np.zeros(max(n, 1), np.uint8)
        _check(self._lib.cv_keystore_add(h, n, _p(seeds) if n else None, _p(pk), _p(st)), "cv_keystore_add")
        return pk[:n], st[:n]

    def contains(self, pk) -> np.ndarray:
        """cv_keystore_contains: pk (n,32) u8 -> found u8[n]."""
        h = self._open()
        pk = _u8(pk).reshape(-1)
        if pk.size % 32:
            raise ValueError("pk must be n x 32 bytes")
        n = pk.size // 32
        found = np.zeros(max(n, 1), np.uint8)
        _check(self._lib.cv_keystore_contains(h, n, _p(pk) if n else None, _p(found)), "cv_keystore_contains")
        return found[:n]

    def sign(self, pk, arena, off, ln):
        """cv_keystore_sign: pk (n,32) u8, arena u8, off u64[n], ln u32[n] -> (sig (n,64) u8, status u8[n]: CV_KS_OK, or
        CV_KS_NO_KEY with a zero signature)."""
        h = self._open()
        off = np.ascontiguousarray(off, dtype=np.uint64)
        ln = np.ascontiguousarray(ln, dtype=np.uint32)
        n = off.shape[0]
        pk = _arr(pk, np.uint8, n, "pk", 32)
        if ln.shape[0] != n:
            raise ValueError("off/len must have n entries")
        arena = _u8(arena) if arena is not None and np.asarray(arena).size else np.zeros(16, np.uint8)
        sig, st = np.zeros((max(n, 1), 64), np.uint8), np.zeros(max(n, 1), np.uint8)
        rc = self._lib.cv_keystore_sign(h, n, _p(pk), _p(arena), arena.size, _p(off), _p(ln), _p(sig), _p(st))
        if rc == -3 and n and _msg_end(self._lib, off, ln) > arena.size:
            raise ValueError("message range exceeds the arena")
        _check(rc, "cv_keystore_sign")
        return sig[:n], st[:n]

    def sign_transactions(self, arena, leaf_off, leaf_len, tx_leaf_begin, pk, tx_sig_begin):
        """cv_sign_transactions: leaves as merkle_tx_ids takes them; pk (nsig,32) u8 cut by tx_sig_begin u32[ntx+1] ->
        (tx_status u8[ntx] CV_ST_*, ids (ntx,32) u8, sig (nsig,64) u8, first_bad u32[ntx])."""
        h = self._open()
        ntx, arena, leaf_off, leaf_len, tx_leaf_begin = Engine._merkle_args(arena, leaf_off, leaf_len, tx_leaf_begin)
        if ntx < 0:
            raise ValueError("tx_leaf_begin must have ntx + 1 entries")
        tx_sig_begin = _arr(tx_sig_begin, np.uint32, ntx + 1, "tx_sig_begin")
        nsig = int(tx_sig_begin[-1])
        pk = _arr(pk, np.uint8, nsig, "pk", 32)
        st, ids = np.zeros(max(ntx, 1), np.uint8), np.zeros((max(ntx, 1), 32), np.uint8)
        sig, fb = np.zeros((max(nsig, 1), 64), np.uint8), np.zeros(max(ntx, 1), np.uint32)
        rc = self._lib.cv_sign_transactions(self._engine._h, h, ntx, _p(arena), arena.size, _p(leaf_off), _p(leaf_len),
                                            _p(tx_leaf_begin), nsig, _p(pk), _p(tx_sig_begin), _p(st), _p(ids), _p(sig),
                                            _p(fb))
        self._engine._bounded_rc(rc, "cv_sign_transactions", (arena, leaf_off, leaf_len, tx_leaf_begin))
        return st[:ntx], ids[:ntx], sig[:nsig], fb[:ntx]

    def reserve(self, capacity: int):
        _check(self._lib.cv_keystore_reserve(self._open(), int(capacity)), "cv_keystore_reserve")

    def stats(self) -> dict:
        out = np.zeros(len(CV_KS_STATS), np.uint64)
        _check(self._lib.cv_keystore_stats(self._open(), _p(out), out.size), "cv_keystore_stats")
        return dict(zip(CV_KS_STATS, map(int, out)))


class UniquenessSet(_Handle):
    """A device-resident set of consumed states bound to an engine (cv_uniq): the notary's commit step,
    UniquenessProvider.commit (UniquenessProvider.kt:13-35) as InMemoryUniquenessProvider.kt:14-36 decides it, for
    a whole batch in one call.  Keys are 32 bytes, a consuming record is (tx id[32], input index u32, caller u32).
    Calls serialise on the set's own lock.  close() (or the with-statement) frees the table; the engine closes the
    sets still open when it is closed itself."""

    _close_fn, _what = "cv_uniq_close", "uniqueness set"

    def __init__(self, engine: Engine, capacity: int, device: int = 0):
        self._engine = engine
        self._lib = engine._lib
        h = _vp()
        _check(self._lib.cv_uniq_open(engine._h, device, int(capacity), ctypes.byref(h)), "cv_uniq_open")
        self._h = h
        engine._signers.add(self)

    def commit_batch(self, state_key, tx_state_begin, tx_id, caller, tx_enable=None, out=None):
        """cv_uniq_commit_batch: state_key (nstates,32) u8 cut by tx_state_begin u32[ntx+1], tx_id (ntx,32) u8,
        caller u32[ntx], tx_enable u8[ntx] or None -> (tx_status u8[ntx], state_conflict u8[nstates], consumed_id
        (nstates,32) u8, consumed_index u32[nstates], consumed_caller u32[nstates]), decided as ntx sequential
        commits.  CvError with code -4 when the set would pass its capacity: nothing changed, reserve() first.
        out: the five output arrays to write into (default: fresh ones)."""
        h = self._open()
        tx_state_begin = np.ascontiguousarray(tx_state_begin, dtype=np.uint32)
        ntx = tx_state_begin.shape[0] - 1
        if ntx < 0:
            raise ValueError("tx_state_begin must have ntx + 1 entries")
        ns = int(tx_state_begin[-1])
        state_key = _u8(state_key)
        tx_id = _u8(tx_id)
        caller = np.ascontiguousarray(caller, dtype=np.uint32)
        if state_key.size < 32 * ns or tx_id.size < 32 * ntx or caller.shape[0] < ntx:
            raise ValueError("the ranges reach past state_key / tx_id / caller")
        if tx_enable is not None:
            tx_enable = np.ascontiguousarray(tx_enable, dtype=np.uint8)
            if tx_enable.shape[0] < ntx:
                raise ValueError("tx_enable must have one entry per request")
        if state_key.size == 0:
            state_key = np.zeros(32, np.uint8)
        if out is None:
            m = max(ns, 1)
            out = (np.zeros(max(ntx, 1), np.uint8), np.zeros(m, np.uint8), np.zeros((m, 32), np.uint8),
                   np.zeros(m, np.uint32), np.zeros(m, np.uint32))
        _check(self._lib.cv_uniq_commit_batch(h, ntx, _p(state_key), _p(tx_state_begin), _p(tx_id), _p(caller),
                                              _p(tx_enable), *[_p(a) for a in out]), "cv_uniq_commit_batch")
        st, sc, cid, cix, cc = out
        return st[:ntx], sc[:ns], cid[:ns], cix[:ns], cc[:ns]

    def lookup(self, state_key):
        """cv_uniq_lookup: state_key (n,32) u8 -> (found u8[n], consumed_id (n,32), consumed_index, consumed_caller)."""
        h = self._open()
        state_key = _u8(state_key)
        n = state_key.size // 32
        m = max(n, 1)
        found, cid = np.zeros(m, np.uint8), np.zeros((m, 32), np.uint8)
        cix, cc = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        _check(self._lib.cv_uniq_lookup(h, n, _p(state_key), _p(found), _p(cid), _p(cix), _p(cc)), "cv_uniq_lookup")
        return found[:n], cid[:n], cix[:n], cc[:n]

    def load(self, state_key, consumed_id, consumed_index, consumed_caller):
        """cv_uniq_load: n rows of a durable log into the set; CvError -3 (the set unchanged) if a key repeats in
        the call or is resident, -4 past the capacity."""
        h = self._open()
        state_key = _u8(state_key)
        consumed_id = _u8(consumed_id)
        n = state_key.size // 32
        consumed_index = np.ascontiguousarray(consumed_index, dtype=np.uint32)
        consumed_caller = np.ascontiguousarray(consumed_caller, dtype=np.uint32)
        if consumed_id.size != 32 * n or consumed_index.shape[0] != n or consumed_caller.shape[0] != n:
            raise ValueError("one id, index and caller per key")
        _check(self._lib.cv_uniq_load(h, n, _p(state_key), _p(consumed_id), _p(consumed_index), _p(consumed_caller)),
               "cv_uniq_load")

    def snapshot_chunks(self, max_entries: int):
        """One pass of cv_uniq_snapshot (DistributedImmutableMap.snapshot) as a generator of (state_key (k,32) u8,
        consumed_id (k,32) u8, consumed_index u32[k], consumed_caller u32[k]) chunks of at most max_entries records,
        in the table's slot order; chunks may be empty.  A call that changes the set between two chunks ends the pass
        with CvError -3."""
        m = int(max_entries)
        if m < 1:
            raise ValueError("max_entries must be at least 1")
        cursor = np.zeros(2, np.uint64)
        key, cid = np.zeros((m, 32), np.uint8), np.zeros((m, 32), np.uint8)
        cix, cc = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        n = _sz(0)
        while int(cursor[0]) != 0xFFFFFFFFFFFFFFFF:
            _check(self._lib.cv_uniq_snapshot(self._open(), _p(cursor), m, _p(key), _p(cid), _p(cix), _p(cc),
                                              ctypes.byref(n)), "cv_uniq_snapshot")
            k = n.value
            yield key[:k].copy(), cid[:k].copy(), cix[:k].copy(), cc[:k].copy()

    def snapshot(self, max_entries=None):
        """Every entry of the set: (state_key (n,32) u8, consumed_id (n,32) u8, consumed_index u32[n], consumed_caller
        u32[n]) of one whole pass, in the table's slot order.  max_entries: the records per call of a chunked pass
        (default: room for every resident entry)."""
        m = max(self.stats()["resident"], 1) if max_entries is None else int(max_entries)
        parts = list(self.snapshot_chunks(m))
        if not parts:
            return np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        return tuple(np.concatenate([p[j] for p in parts]) for j in range(4))

    def clear(self):
        """cv_uniq_clear (map.clear()): the set is empty afterwards; capacity and slots are kept."""
        _check(self._lib.cv_uniq_clear(self._open()), "cv_uniq_clear")

    def install(self, state_key, consumed_id, consumed_index, consumed_caller):
        """cv_uniq_install (DistributedImmutableMap.install): the set holds exactly these n entries afterwards;
        CvError -3 with the set unchanged if a key repeats."""
        h = self._open()
        state_key = _u8(state_key)
        consumed_id = _u8(consumed_id)
        n = state_key.size // 32
        consumed_index = np.ascontiguousarray(consumed_index, dtype=np.uint32)
        consumed_caller = np.ascontiguousarray(consumed_caller, dtype=np.uint32)
        if consumed_id.size != 32 * n or consumed_index.shape[0] != n or consumed_caller.shape[0] != n:
            raise ValueError("one id, index and caller per key")
        _check(self._lib.cv_uniq_install(h, n, _p(state_key), _p(consumed_id), _p(consumed_index), _p(consumed_caller)),
               "cv_uniq_install")

    def reserve(self, capacity: int):
        _check(self._lib.cv_uniq_reserve(self._open(), int(capacity)), "cv_uniq_reserve")

    def set_max_rounds(self, rounds: int):
        _check(self._lib.cv_uniq_set_max_rounds(self._open(), int(rounds)), "cv_uniq_set_max_rounds")

    def stats(self) -> dict:
        """cv_uniq_stats (diagnostics): resident, capacity, slots, rounds and tail of the last commit, probe, wraps."""
        out = np.zeros(len(CV_UNIQ_STATS), np.uint64)
        _check(self._lib.cv_uniq_stats(self._open(), _p(out), out.shape[0]), "cv_uniq_stats")
        return dict(zip(CV_UNIQ_STATS, (int(v) for v in out)))


def dedupe_keys(pk: np.ndarray):
    """The engine's host-side key dedupe (cv_diag_dedupe_keys): (key_index, nkeys) or None when the
    batch would not take the keyed path.  Runs on the host; no device needed."""
    lib = load()
    pk = _u8(pk, 32)
    n = len(pk)
    idx = np.zeros(n, np.uint32)
    nk = ctypes.c_size_t(0)
    rc = lib.cv_diag_dedupe_keys(n, _p(pk), _p(idx), ctypes.byref(nk))
    if rc < 0:
        raise CvError(rc, "cv_diag_dedupe_keys")
    return (idx, int(nk.value)) if rc == 1 else None


def dedupe_keys_workspace(n: int) -> int:
    """Bytes of device workspace Engine.dedupe_keys_device needs for n keys (host only)."""
    return int(load().cv_ed25519_dedupe_keys_workspace(n))


def verify_hotkeys_workspace(n: int) -> int:
    """Bytes of device workspace Engine.verify_device_hotkeys needs for n signatures (host only)."""
    return int(load().cv_ed25519_verify_hotkeys_workspace(n))


def tx_verdicts(bitmap: np.ndarray, tx_sig_begin) -> np.ndarray:
    lib = load()
    tx_sig_begin = np.ascontiguousarray(tx_sig_begin, dtype=np.uint32)
    ntx = tx_sig_begin.shape[0] - 1
    out = np.zeros(max(ntx, 0), np.uint8)
    bitmap = np.ascontiguousarray(bitmap, dtype=np.uint64)
    if bitmap.size == 0:
        bitmap = np.zeros(1, np.uint64)
    _check(lib.cv_tx_verdicts(ntx, _p(bitmap), _p(tx_sig_begin), _p(out)), "cv_tx_verdicts")
    return out


def partial_merkle_build_bound(tx_leaf_begin) -> int:
    """cv_partial_merkle_build_bound: the most nodes the builds of these transactions can emit (host only)."""
    lib = load()
    tx_leaf_begin = np.ascontiguousarray(tx_leaf_begin, dtype=np.uint32)
    ntx = tx_leaf_begin.shape[0] - 1
    return int(lib.cv_partial_merkle_build_bound(ntx, _p(tx_leaf_begin))) if ntx > 0 else 0


def missing_signers_workspace(ntx: int, nnodes: int) -> int:
    """cv_missing_signers_workspace: the bytes of missing_signers_device's d_workspace (host only)."""
    return int(load().cv_missing_signers_workspace(ntx, nnodes))


def bitmap_to_bools(bitmap: np.ndarray, n: int) -> np.ndarray:
    bits = np.unpackbits(np.ascontiguousarray(bitmap, dtype="<u8").view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


_default: Optional[Engine] = None
_default_lock = threading.Lock()


def default_engine() -> Engine:
    """Process-wide engine on all visible GPUs (the JVM shim's "one ctx per process")."""
    global _default
    with _default_lock:
        if _default is None:
            _default = Engine(0)
        return _default
