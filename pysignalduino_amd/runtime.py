"""ctypes binding of libsdx.so (include/sdx.h) + device-buffer plumbing.

PyTorch is used only for device memory and streams (``torch.cuda``); every
byte of demodulation work runs in the hand-written HIP kernels of
``csrc/sdx_kernels.hip``.  There is NO CPU fallback: when the library or a
GPU is missing, :func:`load_library` / :class:`Engine` raise.
"""
from __future__ import annotations

import ctypes
import os
import struct
from ctypes import POINTER, Structure, c_char_p, c_int, c_int32, c_size_t, c_uint32, c_void_p
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import bank as bankmod

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_lib", "libsdx.so")
ABI_VERSION = 14   # include/sdx.h SDX_ABI_VERSION

KIND_MU, KIND_MS, KIND_MC = 0, 1, 2
KIND_MN = 3        # host-side tag for Engine.run (sdx_demod_mn)
ST_OK, ST_RAISED, ST_OVF_TILE, ST_OVF_OUT = 0, 1, 2, 3
RAISE_NAMES = {1: IndexError, 2: AttributeError, 3: ValueError, 4: TypeError, 5: ZeroDivisionError}
RAISE_CONTRACT = 6  # SDX_RAISE_CONTRACT: a general-path limit (include/sdx.h), not a reference outcome
SHORT_MAX = 256    # k_pulses<.., 4 words, 64 messages/tile>
LONG_MAX = 4096    # k_pulses<.., 64 words, 4 messages/tile>
MC_HEX_MAX = 128   # MC_MAXW * 16 hex characters
MN_HEX_MAX = 4096  # SDX_MN_HEX_MAX

DESC_DT = np.dtype([("rec_begin", "<u4"), ("n_rec", "<u2"), ("status", "u1"), ("raise_kind", "u1")])
# sdx_msg_rec (include/sdx.h): one message's header fields, written by sdx_group_pulses
MREC_DT = np.dtype([("off", "<i8"), ("len", "<i4"), ("npat", "u1"), ("cp_slot", "i1"), ("ms_ok", "u1"), ("res0", "u1"),
                    ("pat_id", "u1", (10,)), ("res1", "u1", (6,)), ("pat_val", "<f8", (10,)), ("res2", "u1", (16,))])
MREC_BYTES = 128
RES_DT = np.dtype([("payload_off", "<u4"), ("payload_len", "<u2"), ("proto", "<u2"), ("bit_length", "<u4"),
                   ("msg", "<u4")])

EXPORTED = ["sdx_abi_version", "sdx_last_error", "sdx_source_hash", "sdx_layout_size", "sdx_bank_create", "sdx_bank_destroy",
            "sdx_bank_device_ptr", "sdx_demod_pulses", "sdx_demod_pulses_long", "sdx_demod_mc", "sdx_demod_mn",
            "sdx_parse_lines", "sdx_select_lines", "sdx_serialize_json", "sdx_units",
            "sdx_exchange_work_bytes", "sdx_exchange_send_bytes", "sdx_exchange_count", "sdx_exchange_pack", "sdx_exchange_pack_into", "sdx_exchange_unpack_work_bytes",
            "sdx_exchange_unpack", "sdx_pulses_work_bytes", "sdx_group_work_bytes", "sdx_group_pulses",
            "sdx_general_work_bytes", "sdx_demod_pulses_general", "sdx_mc_general_work_bytes", "sdx_demod_mc_general",
            "sdx_lines_general", "sdx_lines_exact", "sdx_parse_floats", "sdx_format_floats", "sdx_copy_async", "sdx_copy_async_kind", "sdx_copy_async_narrow",
            "sdx_fill_async", "sdx_demod_step", "sdx_group_step", "sdx_split_work_bytes", "sdx_split_lines",
            "sdx_host_count_byte", "sdx_serialize_json_skip", "sdx_mark_repeats", "sdx_repeat_state_bytes",
            "sdx_repeat_scratch_bytes", "sdx_repeat_tile", "sdx_mark_repeats_timed", "sdx_repeat_timed_state_bytes",
            "sdx_repeat_timed_scratch_bytes", "sdx_mark_repeats_by_source", "sdx_repeat_sources_state_bytes",
            "sdx_repeat_sources_scratch_bytes", "sdx_route_table_create", "sdx_route_table_destroy",
            "sdx_route_table_lds_routes", "sdx_route_lines", "sdx_route_records", "sdx_route_skip",
            "sdx_profile_table_create", "sdx_profile_table_destroy", "sdx_profile_check", "sdx_profile_scratch_bytes",
            "sdx_filter_records", "sdx_dispatch_scratch_bytes", "sdx_dispatch_records", "sdx_index_scratch_bytes",
            "sdx_index_records", "sdx_serialize_json_lines"]
REPEAT_SOURCES_MAX = 4096   # SDX_REPEAT_SOURCES_MAX
# sdx_repeat_source_entry (csrc/sdx_repeat_layout.h): a source's slot header after a chunk + its last result-bearing line
REPEAT_SOURCE_ENTRY = np.dtype([("valid", "<u4"), ("kind", "<u4"), ("proto", "<u4"), ("len", "<u4"), ("t", "<i8"),
                                ("last", "<i4"), ("pad", "<i4")])
REPEAT_SLOT_HDR = 24        # sizeof(sdx_repeat_timed_state_hdr): a slot's payload bytes follow it


def _n_sources(sources) -> int:
    s = int(sources)
    if not 1 <= s <= REPEAT_SOURCES_MAX:
        raise ValueError(f"repeat sources: 1 to {REPEAT_SOURCES_MAX}, not {sources}")
    return s


GROUP_MIN = int(os.environ.get("SDX_GROUP_MIN", "4096"))   # SDX_GROUP_MIN (the env: A/B of the grouping)


class SdxPulseBatch(Structure):
    _fields_ = [("data_dev", c_void_p), ("offsets_dev", c_void_p), ("npat_dev", c_void_p),
                ("pat_id_dev", c_void_p), ("pat_val_dev", c_void_p), ("cp_slot_dev", c_void_p),
                ("ms_ok_dev", c_void_p), ("len_dev", c_void_p), ("sel_dev", c_void_p), ("n", c_int32),
                ("n_sel", c_int32), ("mrec_dev", c_void_p)]


class SdxGeneralBatch(Structure):
    _fields_ = [("data_dev", c_void_p), ("offsets_dev", c_void_p), ("npat_dev", c_void_p), ("pat_ids_dev", c_void_p),
                ("pat_val_dev", c_void_p), ("cp_slot_dev", c_void_p), ("ms_ok_dev", c_void_p), ("sel_dev", c_void_p),
                ("n", c_int32), ("n_sel", c_int32), ("len_dev", c_void_p), ("work_stride", ctypes.c_int64),
                ("max_len", c_int32), ("res", c_int32)]


class SdxLinesGeneralOut(Structure):
    _fields_ = [(f, c_void_p) for f in ("offsets_dev", "len_dev", "npat_dev", "pat_ids_dev", "pat_val_dev",
                                         "cp_slot_dev", "ms_ok_dev")]


class SdxMcBatch(Structure):
    _fields_ = [("hex_dev", c_void_p), ("offsets_dev", c_void_p), ("clock_dev", c_void_p),
                ("mcbitnum_dev", c_void_p), ("flags_dev", c_void_p), ("len_dev", c_void_p), ("sel_dev", c_void_p),
                ("n", c_int32), ("n_sel", c_int32), ("only_dev", c_void_p), ("max_hex", c_int32), ("res", c_int32)]


class SdxMnBatch(Structure):
    _fields_ = [("hex_dev", c_void_p), ("offsets_dev", c_void_p), ("len_dev", c_void_p), ("sel_dev", c_void_p),
                ("n", c_int32), ("n_sel", c_int32), ("elig", ctypes.c_uint64), ("method", c_int32), ("res", c_int32)]


class SdxJsonIn(Structure):
    _fields_ = [("kind", c_int32), ("first_only", c_int32), ("desc_dev", c_void_p), ("rec_dev", c_void_p),
                ("cursor_dev", c_void_p), ("heap_dev", c_void_p), ("meta_dev", c_void_p), ("pat_val_dev", c_void_p),
                ("cp_slot_dev", c_void_p), ("n", c_int32), ("rec_max", c_int32)]


class SdxJsonOut(Structure):
    _fields_ = [("json_dev", c_void_p), ("off_dev", c_void_p), ("len_dev", c_void_p), ("cursor_dev", c_void_p),
                ("json_cap", c_uint32), ("res", c_uint32)]


class SdxDispatchRules(Structure):
    """sdx_dispatch_rules (include/sdx.h), 152 bytes: dispatch.DispatchRules.struct fills it."""
    _fields_ = [("keep_equal", (ctypes.c_uint64 * 4) * 4), ("max_repeat", c_int32 * 4), ("drop_equal", c_int32),
                ("res", c_int32)]


class SdxUnitBatch(Structure):
    _fields_ = [("op", c_int32), ("n", c_int32), ("in_dev", c_void_p), ("in_off_dev", c_void_p), ("arg_dev", c_void_p),
                ("val_dev", c_void_p), ("val_off_dev", c_void_p), ("mcrec_dev", c_void_p), ("out_off_dev", c_void_p)]


class SdxXchgPart(Structure):
    _fields_ = [("desc_dev", c_void_p), ("rec_dev", c_void_p), ("heap_dev", c_void_p), ("cursor_dev", c_void_p),
                ("n_msgs", c_uint32), ("rec_cap", c_uint32), ("heap_cap", c_uint32), ("kind", ctypes.c_uint8),
                ("alt", ctypes.c_uint8), ("aux", ctypes.c_uint8), ("res", ctypes.c_uint8),
                ("wire_dev", c_void_p), ("xrec_dev", c_void_p)]


class SdxXchgWire(Structure):
    _fields_ = [("msg_dev", c_void_p), ("rec_dev", c_void_p), ("heap_dev", c_void_p), ("n_msgs", c_uint32),
                ("n_rec", c_uint32), ("n_heap", c_uint32), ("n_payload", c_uint32)]


# the exchange's wire form (include/sdx.h, v3): one word per message, 8 bytes per record, payloads raw or
# as packed hex digits (proto bit 15 = WIRE_NIB: preamble + digits + postamble of the protocol)
WIRE_REC_DT = np.dtype([("proto", "<u2"), ("payload_len", "<u2"), ("bit_length", "<u4")])
WIRE_NIB = 0x8000
XCHG_MAX_RANKS = 32
XCHG_MAX_PARTS = 16
XCHG_COUNTS = 8     # u32 counts per part: messages, records, wire payload bytes, bad, payload bytes, 0, 0, 0
ST_ABSENT = 0xFF    # an exchange overlay's descriptor no re-run wrote
KIND_RAW = 0xFF     # sdx_xchg_part.kind: no affixes (raw payloads only)


class SdxOut(Structure):
    _fields_ = [("desc_dev", c_void_p), ("rec_dev", c_void_p), ("heap_dev", c_void_p), ("cursor_dev", c_void_p),
                ("rec_cap", c_uint32), ("heap_cap", c_uint32), ("work_dev", c_void_p), ("work_cap", ctypes.c_uint64),
                ("wire_dev", c_void_p), ("xrec_dev", c_void_p)]


class SdxStep(Structure):
    _fields_ = [("mu", POINTER(SdxPulseBatch)), ("mu_out", POINTER(SdxOut)), ("ms", POINTER(SdxPulseBatch)),
                ("ms_out", POINTER(SdxOut)), ("mc", POINTER(SdxMcBatch)), ("mc_out", POINTER(SdxOut))]


class SdxGroupJob(Structure):
    _fields_ = [("batch", POINTER(SdxPulseBatch)), ("order_dev", c_void_p), ("mrec_dev", c_void_p),
                ("work_dev", c_void_p), ("work_cap", c_size_t)]


class SdxLines(Structure):
    _fields_ = [("bytes_dev", c_void_p), ("offsets_dev", c_void_p), ("n", c_int32)]


class SdxLinesOut(Structure):
    _fields_ = [(f, c_void_p) for f in ("kind_dev", "status_dev", "slot_dev", "doff_dev", "dlen_dev", "npat_dev",
                                         "pat_id_dev", "pat_val_dev", "cp_slot_dev", "ms_ok_dev", "clock_dev",
                                         "mcbitnum_dev", "mcflags_dev", "meta_dev", "plen_dev")]


# include/sdx.h front-end constants
LINE_NONE, LINE_MU, LINE_MS, LINE_MC, LINE_MN = 0, 1, 2, 3, 4
LS_OK, LS_NOFRAME, LS_NOPARSER, LS_INVALID, LS_NODATA, LS_UNSUPPORTED, LS_RAISES, LS_GENERAL = 0, 1, 2, 3, 4, 5, 6, 7
# (ABI 14: MC lines of <= SDX_MC_SHORT_HEX characters and longer ones are separate classes)
SEL_MU_SHORT, SEL_MU_LONG, SEL_MS_SHORT, SEL_MS_LONG, SEL_MC, SEL_MC_LONG, SEL_MN, SEL_NCLASS = 0, 1, 2, 3, 4, 5, 6, 7
MC_SHORT_HEX = 64   # SDX_MC_SHORT_HEX
SEL_CHUNK = 1024

_LIB = None


def load_library(path: Optional[str] = None):
    """Load libsdx.so (fails loudly -- the product path has no fallback)."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or os.environ.get("SDX_LIB") or LIB_PATH
    # torch bundles its own libamdhip64.so.7: load it FIRST so that libsdx's NEEDED
    # libamdhip64.so.7 resolves to the same runtime (one HIP runtime per process).
    import torch  # noqa: F401
    if not os.path.exists(p):
        raise RuntimeError(f"libsdx.so not built ({p}); run __graft_entry__.build() "
                           "or python -m pysignalduino_amd.build")
    lib = ctypes.CDLL(p)
    lib.sdx_abi_version.restype = c_int
    lib.sdx_last_error.restype = c_char_p
    lib.sdx_source_hash.restype = c_char_p
    lib.sdx_layout_size.argtypes = [c_int]
    lib.sdx_layout_size.restype = c_int
    lib.sdx_copy_async.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.sdx_copy_async.restype = c_int
    lib.sdx_copy_async_kind.argtypes = [c_void_p, c_void_p, c_size_t, c_int, c_void_p]
    lib.sdx_copy_async_kind.restype = c_int
    lib.sdx_copy_async_narrow.argtypes = [c_void_p, c_void_p, c_size_t, c_int, c_void_p]
    lib.sdx_copy_async_narrow.restype = c_int
    lib.sdx_fill_async.argtypes = [c_void_p, c_int, c_size_t, c_void_p]
    lib.sdx_fill_async.restype = c_int
    lib.sdx_bank_create.argtypes = [c_void_p, c_size_t, c_int, POINTER(c_void_p)]
    lib.sdx_bank_create.restype = c_int
    lib.sdx_bank_destroy.argtypes = [c_void_p]
    lib.sdx_bank_destroy.restype = c_int
    lib.sdx_bank_device_ptr.argtypes = [c_void_p]
    lib.sdx_bank_device_ptr.restype = c_void_p
    for fn in ("sdx_demod_pulses", "sdx_demod_pulses_long"):
        f = getattr(lib, fn)
        f.argtypes = [c_void_p, c_int, POINTER(SdxPulseBatch), POINTER(SdxOut), c_void_p]
        f.restype = c_int
    lib.sdx_pulses_work_bytes.argtypes = [c_int]
    lib.sdx_pulses_work_bytes.restype = c_size_t
    lib.sdx_group_work_bytes.argtypes = [c_int]
    lib.sdx_group_work_bytes.restype = c_size_t
    lib.sdx_group_pulses.argtypes = [c_void_p, c_int, POINTER(SdxPulseBatch), c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_void_p]
    lib.sdx_group_pulses.restype = c_int
    lib.sdx_general_work_bytes.argtypes = [c_void_p, c_int, ctypes.c_int64, c_int32, c_int32, ctypes.c_int64]
    lib.sdx_general_work_bytes.restype = ctypes.c_uint64
    lib.sdx_demod_pulses_general.argtypes = [c_void_p, c_int, POINTER(SdxGeneralBatch), POINTER(SdxOut), c_void_p]
    lib.sdx_demod_pulses_general.restype = c_int
    lib.sdx_mc_general_work_bytes.argtypes = [c_int32, c_int32]
    lib.sdx_mc_general_work_bytes.restype = ctypes.c_uint64
    lib.sdx_demod_mc_general.argtypes = [c_void_p, POINTER(SdxMcBatch), c_int32, POINTER(SdxOut), c_void_p]
    lib.sdx_demod_mc_general.restype = c_int
    lib.sdx_lines_general.argtypes = [POINTER(SdxLines), POINTER(SdxLinesOut), c_void_p, c_int32,
                                      POINTER(SdxLinesGeneralOut), c_void_p]
    lib.sdx_lines_general.restype = c_int
    lib.sdx_lines_exact.argtypes = [POINTER(SdxLines), POINTER(SdxLinesOut), c_void_p, c_int32,
                                    POINTER(SdxLinesGeneralOut), c_void_p]
    lib.sdx_lines_exact.restype = c_int
    lib.sdx_parse_floats.argtypes = [POINTER(SdxLines), c_void_p, c_void_p, c_void_p]
    lib.sdx_parse_floats.restype = c_int
    lib.sdx_format_floats.argtypes = [c_void_p, c_int32, c_int32, c_void_p, c_void_p]
    lib.sdx_format_floats.restype = c_int
    lib.sdx_split_work_bytes.argtypes = [ctypes.c_int64]
    lib.sdx_split_work_bytes.restype = c_size_t
    lib.sdx_split_lines.argtypes = [c_void_p, ctypes.c_int64, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
    lib.sdx_split_lines.restype = c_int
    lib.sdx_host_count_byte.argtypes = [c_void_p, ctypes.c_uint64, c_int]
    lib.sdx_host_count_byte.restype = ctypes.c_uint64
    lib.sdx_demod_mc.argtypes = [c_void_p, POINTER(SdxMcBatch), POINTER(SdxOut), c_void_p]
    lib.sdx_group_step.restype = c_int
    lib.sdx_group_step.argtypes = [c_void_p, POINTER(SdxGroupJob), POINTER(SdxGroupJob), c_void_p]
    lib.sdx_demod_step.restype = c_int
    lib.sdx_demod_step.argtypes = [c_void_p, POINTER(SdxStep), c_void_p]
    lib.sdx_demod_mc.restype = c_int
    lib.sdx_demod_mn.argtypes = [c_void_p, POINTER(SdxMnBatch), POINTER(SdxOut), c_void_p]
    lib.sdx_demod_mn.restype = c_int
    lib.sdx_serialize_json.argtypes = [c_void_p, POINTER(SdxJsonIn), POINTER(SdxJsonOut), c_void_p]
    lib.sdx_serialize_json.restype = c_int
    lib.sdx_serialize_json_skip.argtypes = [c_void_p, POINTER(SdxJsonIn), POINTER(SdxJsonOut), c_void_p, c_void_p]
    lib.sdx_serialize_json_skip.restype = c_int
    lib.sdx_mark_repeats.argtypes = [c_void_p, POINTER(SdxJsonIn), c_int, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.sdx_mark_repeats.restype = c_int
    lib.sdx_repeat_state_bytes.argtypes = []
    lib.sdx_repeat_state_bytes.restype = c_size_t
    lib.sdx_repeat_scratch_bytes.argtypes = [c_int32]
    lib.sdx_repeat_scratch_bytes.restype = c_size_t
    lib.sdx_repeat_tile.argtypes = []
    lib.sdx_repeat_tile.restype = c_int
    lib.sdx_mark_repeats_timed.argtypes = [c_void_p, POINTER(SdxJsonIn), c_int, c_int32, c_void_p, ctypes.c_int64, c_void_p,
                                           c_void_p, c_void_p, c_void_p]
    lib.sdx_mark_repeats_timed.restype = c_int
    lib.sdx_repeat_timed_state_bytes.argtypes = []
    lib.sdx_repeat_timed_state_bytes.restype = c_size_t
    lib.sdx_repeat_timed_scratch_bytes.argtypes = [c_int32]
    lib.sdx_repeat_timed_scratch_bytes.restype = c_size_t
    lib.sdx_mark_repeats_by_source.argtypes = [c_void_p, POINTER(SdxJsonIn), c_int, c_int32, c_void_p, c_int32, c_void_p,
                                               ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.sdx_mark_repeats_by_source.restype = c_int
    lib.sdx_repeat_sources_state_bytes.argtypes = [c_int32]
    lib.sdx_repeat_sources_state_bytes.restype = c_size_t
    lib.sdx_repeat_sources_scratch_bytes.argtypes = [c_int32, c_int32]
    lib.sdx_repeat_sources_scratch_bytes.restype = c_size_t
    lib.sdx_route_table_create.argtypes = [c_void_p, c_size_t, c_int, POINTER(c_void_p)]
    lib.sdx_route_table_create.restype = c_int
    lib.sdx_route_table_destroy.argtypes = [c_void_p]
    lib.sdx_route_table_destroy.restype = c_int
    lib.sdx_route_table_lds_routes.argtypes = [c_void_p]
    lib.sdx_route_table_lds_routes.restype = c_int
    lib.sdx_route_lines.argtypes = [c_void_p, c_void_p, POINTER(SdxJsonIn), c_int, c_int32, c_void_p, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p]
    lib.sdx_route_lines.restype = c_int
    lib.sdx_route_records.argtypes = [c_void_p, c_void_p, POINTER(SdxJsonIn), c_int, c_int32, c_void_p, c_void_p, c_void_p,
                                      POINTER(c_void_p), c_void_p]
    lib.sdx_route_records.restype = c_int
    lib.sdx_route_skip.argtypes = [POINTER(SdxJsonIn), c_int, c_int32, c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    lib.sdx_route_skip.restype = c_int
    lib.sdx_profile_table_create.argtypes = [c_void_p, c_size_t, c_int, POINTER(c_void_p)]
    lib.sdx_profile_table_create.restype = c_int
    lib.sdx_profile_table_destroy.argtypes = [c_void_p]
    lib.sdx_profile_table_destroy.restype = c_int
    lib.sdx_profile_check.argtypes = [c_void_p, c_size_t]
    lib.sdx_profile_check.restype = ctypes.c_char_p
    lib.sdx_profile_scratch_bytes.argtypes = [c_int, c_int32]
    lib.sdx_profile_scratch_bytes.restype = c_size_t
    lib.sdx_filter_records.argtypes = [c_void_p, c_void_p, POINTER(SdxJsonIn), c_int, c_int32, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p]
    lib.sdx_filter_records.restype = c_int
    lib.sdx_dispatch_scratch_bytes.argtypes = [c_int, c_int32]
    lib.sdx_dispatch_scratch_bytes.restype = c_size_t
    lib.sdx_dispatch_records.argtypes = [c_void_p, POINTER(SdxDispatchRules), POINTER(SdxJsonIn), c_int, c_int32, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.sdx_dispatch_records.restype = c_int
    lib.sdx_index_scratch_bytes.argtypes = [c_int32]
    lib.sdx_index_scratch_bytes.restype = c_size_t
    lib.sdx_index_records.argtypes = [POINTER(SdxJsonIn), c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.sdx_index_records.restype = c_int
    lib.sdx_serialize_json_lines.argtypes = [c_void_p, POINTER(SdxJsonIn), POINTER(SdxJsonOut), c_void_p, c_uint32, c_void_p]
    lib.sdx_serialize_json_lines.restype = c_int
    lib.sdx_parse_lines.argtypes = [POINTER(SdxLines), POINTER(SdxLinesOut), c_void_p]
    lib.sdx_parse_lines.restype = c_int
    lib.sdx_select_lines.argtypes = [POINTER(SdxLinesOut), c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.sdx_select_lines.restype = c_int
    lib.sdx_units.argtypes = [POINTER(SdxUnitBatch), POINTER(SdxOut), c_void_p]
    lib.sdx_units.restype = c_int
    lib.sdx_exchange_work_bytes.argtypes = [c_void_p, c_int]
    lib.sdx_exchange_work_bytes.restype = ctypes.c_uint64
    lib.sdx_exchange_send_bytes.argtypes = [POINTER(SdxXchgPart), c_int]
    lib.sdx_exchange_send_bytes.restype = ctypes.c_uint64
    lib.sdx_exchange_count.argtypes = [c_void_p, POINTER(SdxXchgPart), c_int, c_void_p, ctypes.c_uint64, c_void_p,
                                       c_void_p]
    lib.sdx_exchange_count.restype = c_int
    lib.sdx_exchange_pack.argtypes = [c_void_p, POINTER(SdxXchgPart), c_int, c_void_p, ctypes.c_uint64, c_void_p,
                                      c_void_p, ctypes.c_uint64, c_void_p]
    lib.sdx_exchange_pack.restype = c_int
    lib.sdx_exchange_pack_into.argtypes = [c_void_p, POINTER(SdxXchgPart), c_int, c_void_p, ctypes.c_uint64, c_void_p,
                                           c_void_p, c_void_p, ctypes.c_uint64, c_void_p]
    lib.sdx_exchange_pack_into.restype = c_int
    lib.sdx_exchange_unpack_work_bytes.argtypes = [c_uint32, c_uint32]
    lib.sdx_exchange_unpack_work_bytes.restype = ctypes.c_uint64
    lib.sdx_exchange_unpack.argtypes = [c_void_p, c_int, POINTER(SdxXchgWire), c_int, c_void_p, ctypes.c_uint64,
                                        c_void_p, c_void_p, c_void_p, ctypes.c_uint64, c_void_p]
    lib.sdx_exchange_unpack.restype = c_int
    if lib.sdx_abi_version() != ABI_VERSION:
        raise RuntimeError("libsdx ABI version mismatch")
    check_layout(lib)
    if path is None:
        _LIB = lib
    return lib


def check_layout(lib) -> None:
    """The numpy mirrors of the C structs must match sizeof() on the C side."""
    want = {0: struct.calcsize(bankmod.HDR_FMT), 1: bankmod.PATSPEC.itemsize, 2: bankmod.MU_REC.itemsize, 3: bankmod.MS_REC.itemsize,
            4: bankmod.MC_REC.itemsize, 5: RES_DT.itemsize, 6: DESC_DT.itemsize, 7: bankmod.MU_DESC.itemsize,
            8: bankmod.MN_REC.itemsize, 9: bankmod.JSON_REC.itemsize, 10: bankmod.MU_FILT.itemsize,
            11: bankmod.MS_FILT.itemsize, 12: ctypes.sizeof(SdxXchgPart), 13: ctypes.sizeof(SdxXchgWire),
            14: WIRE_REC_DT.itemsize, 15: MREC_DT.itemsize, 16: ctypes.sizeof(SdxPulseBatch), 17: ctypes.sizeof(SdxOut)}
    for k, v in want.items():
        got = lib.sdx_layout_size(k)
        if got != v:
            raise RuntimeError(f"struct layout mismatch (item {k}): C {got} vs Python {v}")


def _check(lib, rc):
    if rc != 0:
        raise RuntimeError(f"libsdx error {rc}: {lib.sdx_last_error().decode(errors='replace')}")


def _ptr(t) -> Optional[int]:
    return None if t is None else int(t.data_ptr())


def copy_async(dst, src, stream) -> None:
    """dst.copy_(src, non_blocking=True) on ``stream`` through sdx_copy_async: contiguous tensors of
    the same byte size (device or pinned host), one runtime call instead of a framework dispatch."""
    n = src.numel() * src.element_size()
    if n != dst.numel() * dst.element_size() or not (dst.is_contiguous() and src.is_contiguous()):
        raise ValueError("copy_async: contiguous tensors of the same byte size")
    lib = load_library()
    if _COPY_DEFAULT:
        _check(lib, lib.sdx_copy_async(dst.data_ptr(), src.data_ptr(), n, stream.cuda_stream))
        return
    # the direction named explicitly (hipMemcpyKind): with hipMemcpyDefault the runtime ran the
    # device -> pinned-host copies as blit kernels on every CU (__amd_rocclr_copyBuffer, 256 workgroups
    # held for the PCIe transfer), beside the next chunks' demodulation tiles
    kind = (3 if src.is_cuda else 1) if dst.is_cuda else (2 if src.is_cuda else 0)
    _check(lib, lib.sdx_copy_async_kind(dst.data_ptr(), src.data_ptr(), n, kind, stream.cuda_stream))


_COPY_DEFAULT = os.environ.get("SDX_COPY_DEFAULT") == "1"   # A/B: every copy with hipMemcpyDefault
# copy_d2h's workgroups; 0 (default): hipMemcpyAsync.  16 narrow workgroups measured no faster in the
# streaming front end (profiles/r05/stream/r05k_*: 207 vs 212M lines/s, 64: 178M)
D2H_NARROW_WG = int(os.environ.get("SDX_D2H_WG", "0"))


def copy_d2h(dst, src, stream) -> None:
    """A device -> pinned-host copy that occupies few CUs (sdx_copy_async_narrow, D2H_NARROW_WG
    workgroups): for result copies that run beside demodulation kernels."""
    if D2H_NARROW_WG <= 0 or not dst.is_pinned():
        return copy_async(dst, src, stream)
    n = src.numel() * src.element_size()
    if n != dst.numel() * dst.element_size() or not (dst.is_contiguous() and src.is_contiguous()):
        raise ValueError("copy_d2h: contiguous tensors of the same byte size")
    lib = load_library()
    _check(lib, lib.sdx_copy_async_narrow(dst.data_ptr(), src.data_ptr(), n, D2H_NARROW_WG, stream.cuda_stream))


def fill_async(dst, stream, value: int = 0) -> None:
    """dst.fill_(value) bytewise on ``stream`` through sdx_fill_async (contiguous device tensor)."""
    if not dst.is_contiguous():
        raise ValueError("fill_async: contiguous tensor")
    lib = load_library()
    _check(lib, lib.sdx_fill_async(dst.data_ptr(), int(value), dst.numel() * dst.element_size(), stream.cuda_stream))


class DeviceRouteTable:
    """A route table on the device (sdx_route_table_create): ``handle``, ``table`` (the routes.RouteTable),
    ``lds_routes`` (how many of its routes the kernel serves from LDS).  A blob the host validator refuses
    raises RuntimeError and uploads nothing."""

    def __init__(self, eng: "Engine", table):
        self.lib, self.table = eng.lib, table
        h = c_void_p()
        buf = ctypes.create_string_buffer(table.blob, len(table.blob))
        with eng.torch.cuda.device(eng.device):
            _check(self.lib, self.lib.sdx_route_table_create(ctypes.cast(buf, c_void_p), len(table.blob), eng.device,
                                                             ctypes.byref(h)))
        self.handle = h
        self.lds_routes = int(self.lib.sdx_route_table_lds_routes(h))

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.sdx_route_table_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class DeviceProfileTable:
    """A receiver-profile table on the device (sdx_profile_table_create): ``handle``, ``profiles`` (the
    profiles.ReceiverProfiles).  A blob the host validator refuses raises RuntimeError and uploads nothing."""

    def __init__(self, eng: "Engine", rp, blob: Optional[bytes] = None):
        self.lib, self.profiles = eng.lib, rp
        blob = rp.blob(eng.bank) if blob is None else blob
        h = c_void_p()
        buf = ctypes.create_string_buffer(blob, len(blob))
        with eng.torch.cuda.device(eng.device):
            _check(self.lib, self.lib.sdx_profile_table_create(ctypes.cast(buf, c_void_p), len(blob), eng.device,
                                                               ctypes.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.sdx_profile_table_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def profile_check(blob: bytes) -> Optional[str]:
    """The host validator of a profile table's blob (sdx_profile_validate; no device): None = good, otherwise why
    it is refused."""
    lib = load_library()
    buf = ctypes.create_string_buffer(blob, len(blob))
    why = lib.sdx_profile_check(ctypes.cast(buf, c_void_p), len(blob))
    return None if why is None else why.decode()


class Engine:
    """One device + one uploaded bank.  All launches go to the caller's (torch) stream."""

    def __init__(self, bank: "bankmod.Bank", device: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("pysignalduino_amd needs a ROCm GPU (MI355X); no CPU fallback exists")
        self.torch = torch
        self.lib = load_library()
        self.bank = bank
        self.device = device
        self.dev = torch.device("cuda", device)
        # message records (sdx_msg_rec): the grouping writes them and k_pulses reads its header
        # fields from them.  Off by default: 18 % / 44 % less HBM traffic for k_pulses<MU> / <MS>,
        # but 3.5 % slower on the bench corpus; SDX_MREC=1 turns them on
        self.use_mrec = os.environ.get("SDX_MREC", "0") == "1"
        h = c_void_p()
        blob = ctypes.create_string_buffer(bank.blob, len(bank.blob))
        with torch.cuda.device(device):
            _check(self.lib, self.lib.sdx_bank_create(ctypes.cast(blob, c_void_p), len(bank.blob), device,
                                                      ctypes.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.sdx_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- buffers --------------------------------------------------------------------------------
    def to_device_pulses(self, pb) -> Dict[str, "object"]:
        t = self.torch
        d = self.dev
        out = {
            "data": t.from_numpy(np.ascontiguousarray(pb.data) if len(pb.data) else np.zeros(1, np.uint8)).to(d),
            "offsets": t.from_numpy(np.ascontiguousarray(pb.offsets, dtype=np.int64)).to(d),
            "npat": t.from_numpy(np.ascontiguousarray(pb.npat, dtype=np.uint8)).to(d),
            "pat_id": t.from_numpy(np.ascontiguousarray(pb.pat_id, dtype=np.uint8)).to(d),
            "pat_val": t.from_numpy(np.ascontiguousarray(pb.pat_val, dtype=np.float64)).to(d),
            "cp_slot": t.from_numpy(np.ascontiguousarray(pb.cp_slot, dtype=np.int8)).to(d),
            "ms_ok": t.from_numpy(np.ascontiguousarray(pb.ms_ok, dtype=np.uint8)).to(d),
            "n": int(pb.n),
            "lengths": np.diff(pb.offsets),
        }
        return out

    def to_device_mc(self, mb) -> Dict[str, "object"]:
        t = self.torch
        d = self.dev
        flags = (mb.mtype.astype(np.uint8) & 1) | ((mb.v32.astype(np.uint8) & 1) << 1)
        return {
            # 16 bytes of slack: k_mc stages frames with aligned 8-byte loads (include/sdx.h)
            "hex": t.from_numpy(np.concatenate([np.asarray(mb.hexdata, np.uint8), np.zeros(16, np.uint8)])).to(d),
            "offsets": t.from_numpy(np.ascontiguousarray(mb.offsets, dtype=np.int64)).to(d),
            "clock": t.from_numpy(np.ascontiguousarray(mb.clock, dtype=np.int32)).to(d),
            "mcbitnum": t.from_numpy(np.ascontiguousarray(mb.mcbitnum, dtype=np.int32)).to(d),
            "flags": t.from_numpy(np.ascontiguousarray(flags, dtype=np.uint8)).to(d),
            "n": int(mb.n),
            "lengths": np.diff(mb.offsets),
            # every frame's length is known here: sdx_demod_mc skips its long-frame launch when none
            # is longer than SDX_MC_SHORT_HEX (ABI 13)
            "max_hex": int(np.diff(mb.offsets).max(initial=0)),
        }

    def pulses_work_bytes(self, n: int, spill_frac: float = 0.5) -> int:
        """Workspace of an MU/MS launch over n messages: spill room for `spill_frac` of its
        64-message tiles (a grouped order makes tiles of result-heavy messages)."""
        tiles = (n + 63) // 64
        region = int(self.lib.sdx_pulses_work_bytes(1))
        most = (2 ** 32 - 2 * region) // region          # spill offsets are 32-bit (include/sdx.h)
        return int(self.lib.sdx_pulses_work_bytes(int(min(most, max(16, spill_frac * tiles)))))

    def group_buffers(self, n: int, n_batch: Optional[int] = None):
        """(order, work, mrec) device buffers for sdx_group_pulses over n messages of a batch of
        n_batch (default n): mrec holds one 128-byte sdx_msg_rec per batch message."""
        t = self.torch
        nb = n if n_batch is None else n_batch
        mrec = t.empty(max(nb, 1) * MREC_BYTES + 128, dtype=t.uint8, device=self.dev)
        off = (-mrec.data_ptr()) % 128  # 128-byte aligned records
        return (t.empty(max(n, 1), dtype=t.int32, device=self.dev),
                t.empty(max(int(self.lib.sdx_group_work_bytes(int(n))), 1), dtype=t.uint8, device=self.dev),
                mrec[off: off + max(nb, 1) * MREC_BYTES])

    def group(self, kind: int, bd, sel=None, bufs=None):
        """The grouped message order of a batch (or of `sel`) as a device int32 tensor: the sel of
        the launch_pulses that follows (same results, fewer instructions; sdx_group.hip).  `bufs`:
        group_buffers() to use; default: a per-engine cache (one stream at a time).  The grouping
        also writes the batch's message records into bufs[2] (launch_pulses(mrec=...))."""
        n = int(sel.numel()) if sel is not None else bd["n"]
        if bufs is None:
            c = getattr(self, "_gcache", None)
            if c is None or c[0].numel() < n or c[2].numel() < bd["n"] * MREC_BYTES:
                c = self._gcache = self.group_buffers(n, max(n, bd["n"]))
            bufs = c
        order, work, mrec = bufs
        b = self._pulse_batch(bd, sel)
        um = self.use_mrec   # bool, or the set of kinds whose grouping writes message records
        want = um if isinstance(um, bool) else kind in um
        _check(self.lib, self.lib.sdx_group_pulses(self.handle, kind, ctypes.byref(b), _ptr(order),
                                                   _ptr(mrec) if want else None, _ptr(work),
                                                   int(work.numel()), self.stream_ptr()))
        return order[:n]

    def group_step(self, mu_bd, ms_bd, mu_bufs, ms_bufs, mu_sel=None, ms_sel=None):
        """The MU and MS groupings of one mixed step in the same launches (sdx_group_step, ABI 14): the
        orders group(KIND_MU, ...) and group(KIND_MS, ...) return, as (mu_order, ms_order)."""
        um = self.use_mrec
        jobs, keep = [], []
        for kind, bd, bufs, sel in ((KIND_MU, mu_bd, mu_bufs, mu_sel), (KIND_MS, ms_bd, ms_bufs, ms_sel)):
            order, work, mrec = bufs
            b = self._pulse_batch(bd, sel)
            want = um if isinstance(um, bool) else kind in um
            keep.append(b)
            jobs.append(SdxGroupJob(ctypes.pointer(b), _ptr(order), _ptr(mrec) if want else None, _ptr(work),
                                    int(work.numel())))
        _check(self.lib, self.lib.sdx_group_step(self.handle, ctypes.byref(jobs[0]), ctypes.byref(jobs[1]),
                                                 self.stream_ptr()))
        n_mu = int(mu_sel.numel()) if mu_sel is not None else mu_bd["n"]
        n_ms = int(ms_sel.numel()) if ms_sel is not None else ms_bd["n"]
        return mu_bufs[0][:n_mu], ms_bufs[0][:n_ms]

    def alloc_out(self, n: int, rec_cap: int, heap_cap: int, work_bytes: int = 0, wire: bool = False):
        """Output buffers of one launch.  ``wire``: also the exchange's per-message counts and
        per-record classes (sdx_out.wire_dev / xrec_dev, ABI 12), written by the kernels' flushes so
        that sdx_exchange_count / _pack need not re-read the payloads."""
        t = self.torch
        d = self.dev
        return {
            "desc": t.zeros(max(n, 1) * DESC_DT.itemsize, dtype=t.uint8, device=d),
            "rec": t.empty(max(rec_cap, 1) * RES_DT.itemsize, dtype=t.uint8, device=d),
            "heap": t.empty(max(heap_cap, 1), dtype=t.uint8, device=d),
            "cursor": t.zeros(4, dtype=t.int32, device=d),
            "work": t.empty(work_bytes, dtype=t.uint8, device=d) if work_bytes else None,
            "wire": t.zeros(max(n, 1), dtype=t.int64, device=d) if wire else None,
            "xrec": t.empty(max(rec_cap, 1), dtype=t.int32, device=d) if wire else None,
            "rec_cap": rec_cap, "heap_cap": heap_cap, "n": n,
        }

    @staticmethod
    def _out_struct(o) -> SdxOut:
        w = o.get("work")
        return SdxOut(_ptr(o["desc"]), _ptr(o["rec"]), _ptr(o["heap"]), _ptr(o["cursor"]), o["rec_cap"],
                      o["heap_cap"], _ptr(w), 0 if w is None else int(w.numel()), _ptr(o.get("wire")),
                      _ptr(o.get("xrec")))

    def stream_ptr(self):
        return c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    # -- launches -------------------------------------------------------------------------------
    @staticmethod
    def _pulse_batch(bd, sel, mrec=None) -> SdxPulseBatch:
        return SdxPulseBatch(_ptr(bd["data"]), _ptr(bd["offsets"]), _ptr(bd["npat"]), _ptr(bd["pat_id"]),
                             _ptr(bd["pat_val"]), _ptr(bd["cp_slot"]), _ptr(bd["ms_ok"]), _ptr(bd.get("len")),
                             _ptr(sel), bd["n"], 0 if sel is None else int(sel.numel()), _ptr(mrec))

    def launch_pulses(self, kind: int, bd, out, sel=None, long_variant: bool = False, group: bool = True,
                      mrec=None) -> None:
        """MU/MS launch; the short variant runs batches of >= GROUP_MIN messages in the grouped
        order (group()) unless `group` is False (`sel` then runs in its own order).  `mrec`: the
        message records a group() call wrote for this batch (its bufs[2]), read by the short
        variant instead of the scattered SoA fields."""
        n = int(sel.numel()) if sel is not None else bd["n"]
        if group and not long_variant and n >= GROUP_MIN:
            sel = self.group(kind, bd, sel)
            um = self.use_mrec
            mrec = self._gcache[2] if (um if isinstance(um, bool) else kind in um) else None
        b = self._pulse_batch(bd, sel, None if long_variant else mrec)
        o = self._out_struct(out)
        fn = self.lib.sdx_demod_pulses_long if long_variant else self.lib.sdx_demod_pulses
        _check(self.lib, fn(self.handle, kind, ctypes.byref(b), ctypes.byref(o), self.stream_ptr()))

    @staticmethod
    def _mc_batch(bd, sel) -> SdxMcBatch:
        return SdxMcBatch(_ptr(bd["hex"]), _ptr(bd["offsets"]), _ptr(bd["clock"]), _ptr(bd["mcbitnum"]),
                          _ptr(bd["flags"]), _ptr(bd.get("len")), _ptr(sel), bd["n"],
                          0 if sel is None else int(sel.numel()), _ptr(bd.get("only")), int(bd.get("max_hex", 0)), 0)

    def launch_mc(self, bd, out, sel=None) -> None:
        b = self._mc_batch(bd, sel)
        o = self._out_struct(out)
        _check(self.lib, self.lib.sdx_demod_mc(self.handle, ctypes.byref(b), ctypes.byref(o), self.stream_ptr()))

    def launch_step(self, mu=None, ms=None, mc=None) -> None:
        """One mixed step as one kernel (sdx_demod_step, ABI 14): ``mu`` / ``ms`` = (batch, out, sel,
        mrec) and ``mc`` = (batch, out, sel), each optional; the same results as launch_pulses(MU,
        group=False), launch_pulses(MS, group=False) and launch_mc on the current stream.  The caller
        groups (``sel`` = group()'s order): the fused launch takes its kinds' orders as given."""
        keep = []
        st = SdxStep()
        for name, part in (("mu", mu), ("ms", ms)):
            if part is not None:
                bd, out, sel, mrec = part
                b, o = self._pulse_batch(bd, sel, mrec), self._out_struct(out)
                keep += [b, o]
                setattr(st, name, ctypes.pointer(b))
                setattr(st, name + "_out", ctypes.pointer(o))
        if mc is not None:
            bd, out, sel = mc
            b, o = self._mc_batch(bd, sel), self._out_struct(out)
            keep += [b, o]
            st.mc, st.mc_out = ctypes.pointer(b), ctypes.pointer(o)
        _check(self.lib, self.lib.sdx_demod_step(self.handle, ctypes.byref(st), self.stream_ptr()))

    def launch_mc_general(self, bd, out, sel, max_hex: int) -> None:
        """sdx_demod_mc_general over `sel` (frames of any length; its own bit workspace)."""
        wb = int(self.lib.sdx_mc_general_work_bytes(int(sel.numel()), int(max_hex)))
        work = self.torch.empty(max(wb, 1), dtype=self.torch.uint8, device=self.dev)
        b = SdxMcBatch(_ptr(bd["hex"]), _ptr(bd["offsets"]), _ptr(bd["clock"]), _ptr(bd["mcbitnum"]),
                       _ptr(bd["flags"]), _ptr(bd.get("len")), _ptr(sel), bd["n"], int(sel.numel()),
                       _ptr(bd.get("only")))
        o = self._out_struct(out)
        o.work_dev, o.work_cap = _ptr(work), wb
        _check(self.lib, self.lib.sdx_demod_mc_general(self.handle, ctypes.byref(b), int(max_hex), ctypes.byref(o),
                                                       self.stream_ptr()))
        out["_mcg_work"] = work   # alive until the launch has run (the caller's fetch synchronises)

    # -- general path (sdx_demod_pulses_general) --------------------------------------------------
    def to_device_general(self, arrs) -> Dict[str, "object"]:
        t, d = self.torch, self.dev
        data = arrs["data"] if len(arrs["data"]) else np.zeros(1, np.uint8)
        out = {k: t.from_numpy(np.ascontiguousarray(v)).to(d) for k, v in arrs.items() if k != "data"}
        out["data"] = t.from_numpy(np.ascontiguousarray(data)).to(d)
        out["n"] = int(len(arrs["npat"]))
        out["total"] = int(arrs["offsets"][-1])
        out["lengths"] = np.diff(arrs["offsets"])
        return out

    def run_general(self, kind: int, gd, work_stride: int = 0, rec_cap: Optional[int] = None,
                    heap_cap: Optional[int] = None):
        """MU/MS messages on the general path; returns host (desc, rec, heap) like run().
        ``work_stride`` > 0: per-message scratch of that many bytes (gd in slot layout, "len" set).
        ``rec_cap`` / ``heap_cap``: the first attempt's output capacities (default: sized by the batch);
        an overflow re-runs the batch with both grown."""
        n = gd["n"]
        rec_cap = 16 * n + 1024 if rec_cap is None else int(rec_cap)
        heap_cap = int(2 * gd["total"] + 256 * n + 65536) if heap_cap is None else int(heap_cap)
        lens = gd["lens_host"] if "lens_host" in gd else np.asarray(gd["lengths"])
        max_len = int(lens.max(initial=0))
        wb = int(self.lib.sdx_general_work_bytes(self.handle, kind, int(gd["total"]), n, max_len, int(work_stride)))
        work = self.torch.empty(max(wb, 1), dtype=self.torch.uint8, device=self.dev)
        # the longest messages first: the device's work queue then ends on short ones
        order = np.argsort(-lens, kind="stable").astype(np.int32)
        sel = self.torch.from_numpy(order).to(self.dev)
        for attempt in range(6):
            out = self.alloc_out(n, rec_cap, heap_cap)
            o = self._out_struct(out)
            o.work_dev, o.work_cap = _ptr(work), int(work.numel())
            b = SdxGeneralBatch(_ptr(gd["data"]), _ptr(gd["offsets"]), _ptr(gd["npat"]), _ptr(gd["pat_ids"]),
                                _ptr(gd["pat_val"]), _ptr(gd["cp_slot"]), _ptr(gd["ms_ok"]), _ptr(sel), n, n,
                                _ptr(gd.get("len")), int(work_stride), max_len, 0)
            _check(self.lib, self.lib.sdx_demod_pulses_general(self.handle, kind, ctypes.byref(b), ctypes.byref(o),
                                                               self.stream_ptr()))
            desc, rec, heap = self.fetch(out)
            if not (desc["status"] == ST_OVF_OUT).any():
                return desc, rec, heap
            rec_cap, heap_cap = 4 * rec_cap, 4 * heap_cap   # whole-batch re-run with grown outputs
        raise RuntimeError("general path: result capacity overflow persists")

    def general_overlay(self, kind: int, gd, rows: np.ndarray, work_stride: int = 0):
        """The general path over the messages ``rows`` of a general batch ``gd`` that holds every
        message of a launch (placeholders elsewhere), into an exchange overlay indexed like that
        launch (descriptors of the other messages stay ST_ABSENT).  Capacity overflows re-run the
        launch with grown outputs until none is left (host checks; the general path is rare)."""
        rows = np.asarray(rows, np.int32)
        n = gd["n"]
        lens = np.asarray(gd["lengths"])[rows]
        rec_cap = 16 * len(rows) + 1024
        heap_cap = int(2 * int(lens.sum()) + 256 * len(rows) + 65536)
        max_len = int(lens.max(initial=0))
        wb = int(self.lib.sdx_general_work_bytes(self.handle, kind, int(gd["total"]), n, max_len, int(work_stride)))
        work = self.torch.empty(max(wb, 1), dtype=self.torch.uint8, device=self.dev)
        # the longest messages first: the device's work queue then ends on short ones
        order = rows[np.argsort(-lens, kind="stable")].astype(np.int32)
        sel = self.torch.from_numpy(order).to(self.dev)
        for attempt in range(6):
            out = self.overlay_out(n, rec_cap, heap_cap)
            o = self._out_struct(out)
            o.work_dev, o.work_cap = _ptr(work), int(work.numel())
            b = SdxGeneralBatch(_ptr(gd["data"]), _ptr(gd["offsets"]), _ptr(gd["npat"]), _ptr(gd["pat_ids"]),
                                _ptr(gd["pat_val"]), _ptr(gd["cp_slot"]), _ptr(gd["ms_ok"]), _ptr(sel), n,
                                len(order), _ptr(gd.get("len")), int(work_stride), max_len, 0)
            _check(self.lib, self.lib.sdx_demod_pulses_general(self.handle, kind, ctypes.byref(b), ctypes.byref(o),
                                                               self.stream_ptr()))
            self.torch.cuda.current_stream(self.dev).synchronize()
            st = out["desc"][: n * DESC_DT.itemsize].view(-1, DESC_DT.itemsize)[:, 6].cpu().numpy()[rows]
            if not (st == ST_OVF_OUT).any():
                out["_keep"] = (work, sel)
                return out
            rec_cap, heap_cap = 4 * rec_cap, 4 * heap_cap
        raise RuntimeError("general path: result capacity overflow persists")

    def to_device_mn(self, hexes) -> Dict[str, "object"]:
        """MN frames (hex strings / bytes) -> device batch.  Contract: [0-9A-Fa-f]* and at most
        MN_HEX_MAX characters (checked here; ContractError-free callers check before)."""
        t = self.torch
        bs = [h.encode("latin-1") if isinstance(h, str) else bytes(h) for h in hexes]
        lens = np.fromiter((len(b) for b in bs), np.int64, len(bs))
        offsets = np.zeros(len(bs) + 1, np.int64)
        np.cumsum(lens, out=offsets[1:])
        data = np.concatenate([np.frombuffer(b"".join(bs), np.uint8), np.zeros(16, np.uint8)])  # 8-byte read slack
        return {"hex": t.from_numpy(data).to(self.dev),
                "offsets": t.from_numpy(offsets).to(self.dev), "n": len(bs), "lengths": lens}

    def launch_mn(self, bd, out, elig: int = 0, method: int = -1, sel=None) -> None:
        b = SdxMnBatch(_ptr(bd["hex"]), _ptr(bd["offsets"]), _ptr(bd.get("len")), _ptr(sel), bd["n"],
                       0 if sel is None else int(sel.numel()), elig, method, 0)
        o = self._out_struct(out)
        _check(self.lib, self.lib.sdx_demod_mn(self.handle, ctypes.byref(b), ctypes.byref(o), self.stream_ptr()))

    def split_work_ints(self, nbytes: int) -> int:
        """int32 entries of sdx_split_lines' scratch for a buffer of nbytes."""
        return int(self.lib.sdx_split_work_bytes(int(nbytes))) // 4

    def split_lines(self, bytes_t, nbytes: int, final: bool, offsets_t, cap: int, count_t, scratch_t, stream=None) -> None:
        """sdx_split_lines on ``stream`` (default: the current one; no host sync): the '\\n'-terminated
        lines of bytes_t[:nbytes] -> offsets_t[: cap + 1] (int64), count_t (int64[2]: lines found, start of
        the unterminated tail).  bytes_t holds 16 readable bytes past nbytes."""
        nbytes, cap = int(nbytes), int(cap)
        if (bytes_t.numel() < nbytes + 16 or offsets_t.numel() * offsets_t.element_size() < 8 * (cap + 1) or
                count_t.numel() * count_t.element_size() < 16 or
                scratch_t.numel() * scratch_t.element_size() < 4 * self.split_work_ints(max(nbytes, 0))):
            raise ValueError("split_lines: a buffer is too small for nbytes / cap")
        st = self.stream_ptr() if stream is None else c_void_p(stream.cuda_stream)
        _check(self.lib, self.lib.sdx_split_lines(_ptr(bytes_t), nbytes, 1 if final else 0, _ptr(offsets_t), cap,
                                                  _ptr(count_t), _ptr(scratch_t), st))

    @staticmethod
    def json_in(kind: int, demod_out, lines_out, n: int, first_only=True) -> SdxJsonIn:
        """The sdx_json_in of one demodulation launch (launch_json and mark_repeats take it)."""
        return SdxJsonIn(kind, int(first_only), _ptr(demod_out["desc"]), _ptr(demod_out["rec"]),
                         _ptr(demod_out["cursor"]), _ptr(demod_out["heap"]), _ptr(lines_out["meta"]),
                         _ptr(lines_out.get("pat_val")), _ptr(lines_out.get("cp_slot")), n,
                         0 if first_only else demod_out["rec_cap"])

    def launch_json(self, kind: int, demod_out, lines_out, n: int, jout, first_only: bool = True, skip=None) -> None:
        """sdx_serialize_json over a demodulation launch's device outputs (no host sync).  first_only:
        True / 1 one text per line, 2 the same sparse (only lines with a text are written: launches of
        several kinds share one output), False / 0 one text per record.  ``skip``: a device uint8[n]
        mask (mark_repeats' output): lines with a non-zero entry get no text (sdx_serialize_json_skip)."""
        ji = self.json_in(kind, demod_out, lines_out, n, first_only)
        jo = SdxJsonOut(_ptr(jout["json"]), _ptr(jout["off"]), _ptr(jout["len"]), _ptr(jout["cursor"]),
                        jout["cap"], 0)
        if skip is None:
            _check(self.lib, self.lib.sdx_serialize_json(self.handle, ctypes.byref(ji), ctypes.byref(jo),
                                                         self.stream_ptr()))
            return
        if skip.numel() * skip.element_size() < n:
            raise ValueError("launch_json: skip holds fewer than n bytes")
        _check(self.lib, self.lib.sdx_serialize_json_skip(self.handle, ctypes.byref(ji), ctypes.byref(jo),
                                                          _ptr(skip), self.stream_ptr()))

    # -- repeat suppression (sdx_mark_repeats) -------------------------------------
    def repeat_tile(self) -> int:
        return int(self.lib.sdx_repeat_tile())

    def alloc_repeat_state(self, timed: bool = False, sources: Optional[int] = None):
        """The carried state of one stream of lines, zeroed: no previous result-bearing line.
        ``timed``: the state of mark_repeats_timed (a layout of its own: header, T, payload);
        ``sources``: the state of mark_repeats_by_source, one slot of the timed layout per source id."""
        t = self.torch
        if sources is not None:
            size = self.lib.sdx_repeat_sources_state_bytes(_n_sources(sources))
        else:
            size = self.lib.sdx_repeat_timed_state_bytes() if timed else self.lib.sdx_repeat_state_bytes()
        return t.zeros(int(size), dtype=t.uint8, device=self.dev)

    def _alloc_repeat(self, n: int, scratch_bytes: int):
        t = self.torch
        return (t.zeros(max(n, 1), dtype=t.uint8, device=self.dev), t.empty(int(scratch_bytes), dtype=t.uint8, device=self.dev))

    def _mark(self, name: str, entry, json_ins, n: int, sizes, args, stream, too_small: str = "n") -> None:
        """What the three mark_* methods share.  ``sizes``: (tensor or None, the bytes it must hold) per buffer;
        ``args``: the entry's arguments between n and the stream."""
        if not 1 <= len(json_ins) <= 4:
            raise ValueError(f"{name}: 1 to 4 kinds")
        for x, need in sizes:
            if x is not None and x.numel() * x.element_size() < need:
                raise ValueError(f"{name}: a buffer is too small for {too_small}")
        arr = (SdxJsonIn * len(json_ins))(*json_ins)
        st = self.stream_ptr() if stream is None else c_void_p(stream.cuda_stream)
        _check(self.lib, entry(self.handle, arr, len(json_ins), n, *args, st))

    def alloc_repeat(self, n: int):
        """(repeat mask uint8[n], key scratch) for chunks of up to n lines."""
        return self._alloc_repeat(n, self.lib.sdx_repeat_scratch_bytes(max(n, 1)))

    def mark_repeats(self, json_ins, n: int, repeat, scratch, state, stream=None) -> None:
        """sdx_mark_repeats on ``stream`` (default: the current one; no host sync): repeat[:n] = 1 for the
        lines that repeat the previous result-bearing line's (kind, proto, payload).  ``json_ins``: the
        chunk's SdxJsonIn, one per kind (json_in); ``state``: alloc_repeat_state() of this stream of lines."""
        n, lib = int(n), self.lib
        self._mark("mark_repeats", lib.sdx_mark_repeats, json_ins, n,
                   [(repeat, n), (scratch, lib.sdx_repeat_scratch_bytes(n)), (state, lib.sdx_repeat_state_bytes())],
                   (_ptr(repeat), _ptr(scratch), _ptr(state)), stream)

    def alloc_repeat_timed(self, n: int):
        """(repeat mask uint8[n], scratch) of mark_repeats_timed for chunks of up to n lines."""
        return self._alloc_repeat(n, self.lib.sdx_repeat_timed_scratch_bytes(max(n, 1)))

    def mark_repeats_timed(self, json_ins, n: int, times, window_us: int, repeat, scratch, state, stream=None) -> None:
        """sdx_mark_repeats_timed on ``stream`` (default: the current one; no host sync): mark_repeats where a
        run also ends once its last published line is more than ``window_us`` old.  ``times``: a device
        int64 tensor, one arrival time in microseconds per line, non-decreasing (a precondition the caller
        checks: frontend / stream do); ``scratch``: alloc_repeat_timed's; ``state``:
        alloc_repeat_state(timed=True) of this stream of lines."""
        n, lib = int(n), self.lib
        self._mark("mark_repeats_timed", lib.sdx_mark_repeats_timed, json_ins, n,
                   [(repeat, n), (times, 8 * n), (scratch, lib.sdx_repeat_timed_scratch_bytes(n)),
                    (state, lib.sdx_repeat_timed_state_bytes())],
                   (_ptr(times), int(window_us), _ptr(repeat), _ptr(scratch), _ptr(state)), stream)

    def alloc_repeat_sources(self, n: int, sources: int):
        """(repeat mask uint8[n], scratch) of mark_repeats_by_source for chunks of up to n lines of ``sources`` ids."""
        return self._alloc_repeat(n, self.lib.sdx_repeat_sources_scratch_bytes(max(n, 1), _n_sources(sources)))

    def mark_repeats_by_source(self, json_ins, n: int, source, sources: int, times, window_us, repeat, scratch, state,
                               stream=None) -> None:
        """sdx_mark_repeats_by_source on ``stream`` (default: the current one; no host sync): every source id's
        lines are decided as a stream of their own.  ``source``: a device int32 tensor, one id in
        [0, sources) per line; ``times`` / ``window_us``: as mark_repeats_timed, non-decreasing within each
        source, or None / None for no window (both preconditions are the caller's: frontend / stream check
        them); ``scratch``: alloc_repeat_sources(n, sources)'s; ``state``: alloc_repeat_state(sources=)."""
        n, lib = int(n), self.lib
        ok = 1 <= sources <= REPEAT_SOURCES_MAX    # otherwise the entry refuses the count itself
        self._mark("mark_repeats_by_source", lib.sdx_mark_repeats_by_source, json_ins, n,
                   [(repeat, n), (source, 4 * n), (times, 8 * n), (scratch, lib.sdx_repeat_sources_scratch_bytes(n, sources)),
                    (state, lib.sdx_repeat_sources_state_bytes(sources))] if ok else [],
                   (_ptr(source), int(sources), _ptr(times), 0 if window_us is None else int(window_us), _ptr(repeat),
                    _ptr(scratch), _ptr(state)), stream, "n and sources")

    def repeat_sources_table(self, scratch, sources: int):
        """The compact per-source table mark_repeats_by_source left in ``scratch``: a device uint8 view
        (copy it to the host and read it with REPEAT_SOURCE_ENTRY)."""
        return scratch[16: 16 + REPEAT_SOURCE_ENTRY.itemsize * int(sources)]

    # -- payload routes (sdx_route_lines) --------------------------------------------
    def route_table(self, table) -> "DeviceRouteTable":
        """``table`` (routes.RouteTable, or a list of (name, pattern) pairs) validated and uploaded
        (sdx_route_table_create); the handle is kept on the table object, one per device."""
        from .routes import as_table
        table = as_table(table)
        cache = table.__dict__.setdefault("_device", {})
        if self.device not in cache:
            cache[self.device] = DeviceRouteTable(self, table)
        return cache[self.device]

    def alloc_routes(self, n: int, mask: bool = True, skip: bool = True, pick: bool = False, views: int = 0):
        """{"route": int16[n], "mask": uint64[n] as int64 or None, "skip": uint8[n] or None} for chunks of up to n lines;
        ``pick`` / ``views`` = k add route_records' outputs: "pick" uint16[n] (as int16) and "views", k descriptor
        arrays of 8 n bytes each (uint8)."""
        t, d, n = self.torch, self.dev, max(int(n), 1)
        b = {"route": t.empty(n, dtype=t.int16, device=d), "mask": t.empty(n, dtype=t.int64, device=d) if mask else None,
             "skip": t.empty(n, dtype=t.uint8, device=d) if skip else None}
        if pick:
            b["pick"] = t.empty(n, dtype=t.int16, device=d)
        if views:
            b["views"] = [t.empty(8 * n, dtype=t.uint8, device=d) for _ in range(int(views))]
        return b

    @staticmethod
    def json_in_view(ji: SdxJsonIn, view) -> SdxJsonIn:
        """``ji`` with desc_dev replaced by ``view`` (one of route_records' descriptor arrays): every first_only
        consumer then acts on the line's picked record."""
        out = SdxJsonIn()
        ctypes.memmove(ctypes.byref(out), ctypes.byref(ji), ctypes.sizeof(SdxJsonIn))
        out.desc_dev = _ptr(view)
        return out

    def route_lines(self, table, json_ins, n: int, route, mask=None, skip=None, repeat=None, drop_unrouted: bool = False,
                    stream=None) -> None:
        """sdx_route_lines on ``stream`` (default: the current one; no host sync): route[:n] = the first route
        of ``table`` (route_table's) whose pattern matches the payload of the line's first record, -1 = none
        or no result; mask[:n] (optional) one bit per matching route; skip[:n] (optional) = repeat (optional,
        mark_repeats' mask) or, with ``drop_unrouted``, a result-bearing line without a route -- what
        launch_json takes as ``skip``.  ``json_ins``: the chunk's SdxJsonIn, one per kind (json_in)."""
        n = int(n)
        if not isinstance(table, DeviceRouteTable):
            table = self.route_table(table)
        self._mark("route_lines", lambda bank, arr, k, n_, *a: self.lib.sdx_route_lines(bank, table.handle, arr, k, n_, *a),
                   json_ins, n, [(route, 2 * n), (mask, 8 * n), (skip, n), (repeat, n)],
                   (_ptr(repeat), 1 if drop_unrouted else 0, _ptr(route), _ptr(mask), _ptr(skip)), stream)

    def route_records(self, table, json_ins, n: int, route, pick, views, mask=None, stream=None) -> None:
        """sdx_route_records on ``stream`` (default: the current one; no host sync): pick[:n] = the
        index of the line's first record that some route of ``table`` matches (0: none, or no result), route[:n]
        / mask[:n] (optional) that record's; views[i][:8 n] = json_ins[i]'s descriptors with every result-bearing
        line owning exactly its picked record (json_in_view)."""
        n = int(n)
        if not isinstance(table, DeviceRouteTable):
            table = self.route_table(table)
        if len(views) != len(json_ins):
            raise ValueError("route_records: one view per kind")
        varr = (c_void_p * max(len(views), 1))(*[_ptr(v) for v in views])
        self._mark("route_records", lambda bank, arr, k, n_, *a: self.lib.sdx_route_records(bank, table.handle, arr, k, n_, *a),
                   json_ins, n, [(route, 2 * n), (mask, 8 * n), (pick, 2 * n)] + [(v, 8 * n) for v in views],
                   (_ptr(route), _ptr(mask), _ptr(pick), varr), stream)

    def route_skip(self, json_ins, n: int, route, skip, repeat=None, drop_unrouted: bool = False, stream=None) -> None:
        """sdx_route_skip on ``stream``: skip[:n] = repeat (optional, mark_repeats' mask) or, with ``drop_unrouted``,
        a result-bearing line whose route[:n] entry is negative -- what launch_json takes as ``skip``."""
        n = int(n)
        self._mark("route_skip", lambda bank, arr, k, n_, *a: self.lib.sdx_route_skip(arr, k, n_, *a),
                   json_ins, n, [(route, 2 * n), (skip, n), (repeat, n)],
                   (_ptr(route), _ptr(repeat), 1 if drop_unrouted else 0, _ptr(skip)), stream)

    # -- receiver profiles (sdx_filter_records) -------------------------------------
    def profile_table(self, rp) -> "DeviceProfileTable":
        """``rp`` (profiles.ReceiverProfiles, a Profile or a list of them) compiled against this engine's bank,
        validated and uploaded (sdx_profile_table_create); the handle is kept on the object, one per engine."""
        from .profiles import as_profiles
        rp = as_profiles(rp)
        cache = rp.__dict__.setdefault("_device", {})
        if id(self) not in cache or cache[id(self)][0] is not self:
            cache[id(self)] = (self, DeviceProfileTable(self, rp))
        return cache[id(self)][1]

    def alloc_profiles(self, n: int, outs):
        """The buffers of filter_records for chunks of up to n lines whose launches write ``outs`` (alloc_out's
        dictionaries, one per kind): {"outs": one filtered out per kind -- "desc", "rec" and "cursor" of its own, the
        launch's "heap" and capacities --, "scratch"}."""
        t, d, n = self.torch, self.dev, max(int(n), 1)
        f = []
        for o in outs:
            x = dict(o)
            x.update(desc=t.empty(n * DESC_DT.itemsize, dtype=t.uint8, device=d),
                     rec=t.empty(max(o["rec_cap"], 1) * RES_DT.itemsize, dtype=t.uint8, device=d),
                     cursor=t.zeros(4, dtype=t.int32, device=d), work=None, wire=None, xrec=None)
            f.append(x)
        size = int(self.lib.sdx_profile_scratch_bytes(max(len(outs), 1), n))
        return {"outs": f, "scratch": t.empty(size, dtype=t.uint8, device=d)}

    def filter_records(self, table, json_ins, n: int, bufs, source=None, stream=None, rec_caps=None):
        """sdx_filter_records on ``stream`` (default: the current one; no host sync): the launch outputs behind
        ``json_ins`` (json_in, one per kind) with every line keeping only the records its source's profile enables,
        compacted in line order into ``bufs`` (alloc_profiles').  ``source``: a device int32 tensor, one id per line;
        None = every line is source 0.  ``rec_caps``: the record capacities to declare (default: the buffers').
        Returns bufs["outs"]: filtered outs shaped like alloc_out's, sharing the launches' heaps."""
        if not isinstance(table, DeviceProfileTable):
            table = self.profile_table(table)
        return self._compact("filter_records", self.lib.sdx_filter_records, self.lib.sdx_profile_scratch_bytes,
                             table.handle, json_ins, n, bufs, stream, rec_caps, source)

    def _compact(self, name, entry, scratch_bytes, arg, json_ins, n, bufs, stream, rec_caps, source=False):
        """What filter_records and dispatch_records share: ``entry`` (after the bank: ``arg``, its table or rules)
        over ``json_ins`` into ``bufs``; ``source``: the entry's per-line source ids, False where it takes none."""
        n = int(n)
        outs = bufs["outs"]
        if len(outs) != len(json_ins):
            raise ValueError(name + ": one output per kind")
        k = max(len(outs), 1)
        caps = [o["rec_cap"] for o in outs] if rec_caps is None else [int(c) for c in rec_caps]
        for o, c in zip(outs, caps):
            if o["rec"].numel() < c * RES_DT.itemsize:
                raise ValueError(name + ": a record buffer is smaller than its declared capacity")
        darr = (c_void_p * k)(*[_ptr(o["desc"]) for o in outs])
        rarr = (c_void_p * k)(*[_ptr(o["rec"]) for o in outs])
        carr = (c_void_p * k)(*[_ptr(o["cursor"]) for o in outs])
        caparr = (ctypes.c_uint32 * k)(*caps)
        need = int(scratch_bytes(k, n)) if 1 <= len(outs) <= 4 and n >= 0 else 0
        src = [] if source is False else [(source, 4 * n)]
        self._mark(name, lambda bank, arr, k_, n_, *a: entry(bank, arg, arr, k_, n_, *a),
                   json_ins, n, src + [(bufs["scratch"], need)] + [(o["desc"], 8 * n) for o in outs],
                   (*[_ptr(t_) for t_, _ in src], darr, rarr, caparr, carr, _ptr(bufs["scratch"])), stream)
        return outs

    def filter_fetched(self, table, res: dict, n: int, sources=None) -> dict:
        """filter_records for results already on the host (run()'s): ``res`` maps "MU" / "MS" / "MC" / "MN" to
        (desc, rec, heap) as run() returns them; their descriptors and records go up again, through the pass, and
        come back filtered (the heaps stay: payload offsets are unchanged).  ``sources``: int32[n] or None."""
        src = None if sources is None else self.torch.from_numpy(np.ascontiguousarray(sources, np.int32)).to(self.dev)
        return self._fetched(res, n, False, self.alloc_profiles,
                             lambda ins, bufs: self.filter_records(table, ins, n, bufs, source=src))

    def _fetched(self, res: dict, n: int, heap_up: bool, alloc, run) -> dict:
        """What filter_fetched and dispatch_fetched share: descriptors and records (``heap_up``: and heaps) up,
        ``run(json_ins, alloc(n, outs))``, descriptors and records back."""
        t = self.torch
        names = [k for k in ("MU", "MS", "MC", "MN") if k in res]
        up = lambda a: t.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(self.dev)   # noqa: E731
        outs, ins = [], []
        for name in names:
            desc, rec, heap = res[name]
            o = {"desc": up(desc) if len(desc) else t.zeros(8, dtype=t.uint8, device=self.dev),
                 "rec": up(rec) if len(rec) else t.zeros(RES_DT.itemsize, dtype=t.uint8, device=self.dev),
                 "cursor": t.tensor([len(rec), 0, 0, 0], dtype=t.int32, device=self.dev), "rec_cap": len(rec),
                 "heap_cap": len(heap) if heap_up else 0, "n": n}
            if heap_up:
                o["heap"] = up(heap) if len(heap) else t.zeros(16, dtype=t.uint8, device=self.dev)
            else:
                o["heap"] = o["desc"]    # never read by the pass
            outs.append(o)
            ins.append(self.json_in(("MU", "MS", "MC", "MN").index(name), o, {"meta": o["desc"]}, n))
        f = run(ins, alloc(n, outs))
        out = dict(res)
        for name, o in zip(names, f):
            total = int(o["cursor"][0].item())
            out[name] = (o["desc"][: n * DESC_DT.itemsize].cpu().numpy().view(DESC_DT).copy(),
                         o["rec"][: total * RES_DT.itemsize].cpu().numpy().view(RES_DT).copy(), res[name][2])
        return out

    # -- dispatch rules (sdx_dispatch_records) ----------------------------------------
    def alloc_dispatch(self, n: int, outs):
        """The buffers of dispatch_records for chunks of up to n lines whose launches write ``outs``: 
        alloc_profiles' (sdx_dispatch_scratch_bytes and sdx_profile_scratch_bytes are one formula)."""
        return self.alloc_profiles(n, outs)

    def dispatch_records(self, rules, json_ins, n: int, bufs, stream=None, rec_caps=None):
        """sdx_dispatch_records on ``stream`` (default: the current one; no host sync): the launch outputs behind
        ``json_ins`` (json_in, one per kind) with every line keeping only the records the dispatch rules keep
        (``rules``: a dispatch.DispatchRules, True for the defaults, or a filled SdxDispatchRules), compacted in line
        order into ``bufs`` (alloc_dispatch's).  ``rec_caps``: the record capacities to declare (default: the
        buffers').  Returns bufs["outs"]: reduced outs shaped like alloc_out's, sharing the launches' heaps."""
        if not isinstance(rules, SdxDispatchRules):
            from .dispatch import as_rules
            rules = as_rules(rules)
            if rules is None:
                raise ValueError("dispatch_records: no rules")
            rules = rules.struct(self.bank)
        return self._compact("dispatch_records", self.lib.sdx_dispatch_records, self.lib.sdx_dispatch_scratch_bytes,
                             ctypes.byref(rules), json_ins, n, bufs, stream, rec_caps)

    def dispatch_fetched(self, rules, res: dict, n: int) -> dict:
        """dispatch_records for results already on the host (run()'s), as filter_fetched -- but the heaps go up too:
        this pass reads payloads.  The heaps themselves stay as they are (payload offsets are unchanged)."""
        return self._fetched(res, n, True, self.alloc_dispatch,
                             lambda ins, bufs: self.dispatch_records(rules, ins, n, bufs))

    # -- every message of a line in one chunk result (sdx_index_records) ------------
    def alloc_line_index(self, n: int, rec_max: int, json_cap: Optional[int] = None):
        """The buffers of index_records + launch_json_lines for chunks of up to n lines and ``rec_max`` records over
        all kinds: {"first": int32[n + 1] (uint32 values), "scratch", and alloc_json's "json" / "off" / "len" /
        "cursor" / "cap" with off / len holding ``rec_max`` entries, "rec_max"}.  ``json_cap``: the text buffer's
        bytes (default 256 per record + 64 KB)."""
        t, d, n, rec_max = self.torch, self.dev, max(int(n), 0), max(int(rec_max), 0)
        idx = self.alloc_json(rec_max, 256 * rec_max + 65536 if json_cap is None else int(json_cap))
        # empty, not zeros: index_records writes every entry of first[0, n], and a fill would run on another stream
        idx.update(first=t.empty(n + 1, dtype=t.int32, device=d), rec_max=rec_max, n=n,
                   scratch=t.empty(int(self.lib.sdx_index_scratch_bytes(n)), dtype=t.uint8, device=d))
        return idx

    def index_records(self, json_ins, n: int, idx, skip=None, stream=None) -> None:
        """sdx_index_records on ``stream`` (default: the current one; no host sync): idx["first"][: n + 1] = the
        exclusive prefix, in line order, of every line's record count over ``json_ins`` (json_in, one per kind);
        ``skip``: a device uint8[n] mask (mark_repeats'), a line with a non-zero entry counts 0."""
        n = int(n)
        if not 1 <= len(json_ins) <= 4:
            raise ValueError("index_records: 1 to 4 kinds")
        if n > idx["n"] or (skip is not None and skip.numel() * skip.element_size() < n):
            raise ValueError("index_records: a buffer is too small for n")
        arr = (SdxJsonIn * len(json_ins))(*json_ins)
        st = self.stream_ptr() if stream is None else c_void_p(stream.cuda_stream)
        _check(self.lib, self.lib.sdx_index_records(arr, len(json_ins), n, _ptr(skip), _ptr(idx["first"]),
                                                    _ptr(idx["scratch"]), st))

    def launch_json_lines(self, kind: int, demod_out, lines_out, n: int, idx) -> None:
        """sdx_serialize_json_lines over a demodulation launch's device outputs (no host sync): one text per record
        of the lines index_records counted, its offset and length at the record's chunk index in idx["off"] /
        idx["len"] (alloc_line_index's; the caller zeroes idx["cursor"] once per chunk, all kinds share it)."""
        if n > idx["n"]:
            raise ValueError("launch_json_lines: the index holds fewer than n lines")
        ji = self.json_in(kind, demod_out, lines_out, n, 0)
        jo = SdxJsonOut(_ptr(idx["json"]), _ptr(idx["off"]), _ptr(idx["len"]), _ptr(idx["cursor"]), idx["cap"], 0)
        _check(self.lib, self.lib.sdx_serialize_json_lines(self.handle, ctypes.byref(ji), ctypes.byref(jo),
                                                           _ptr(idx["first"]), idx["rec_max"], self.stream_ptr()))

    def alloc_json(self, items: int, cap: int):
        t, d = self.torch, self.dev
        return {"json": t.empty(max(cap, 8), dtype=t.uint8, device=d), "off": t.empty(max(items, 1), dtype=t.int32, device=d),
                "len": t.empty(max(items, 1), dtype=t.int32, device=d), "cursor": t.zeros(2, dtype=t.int32, device=d),
                "cap": cap, "items": items}

    # -- full run with contract routing and overflow re-runs (all on the GPU) --------------------
    def run(self, kind: int, bd, rec_cap: Optional[int] = None, heap_cap: Optional[int] = None,
            sel_short=None, sel_long=None, mn_elig: int = 0, mn_method: int = -1, workspace: bool = True):
        """Demodulate a device batch; returns host numpy (desc, rec, heap).  The first pass
        (first_pass) then GPU re-runs of overflowed messages (rerun_overlay) merged on the host.

        ``workspace``: MU/MS launches run in the grouped message order with spill regions for
        result-heavy tiles (sdx_group_pulses, sdx_demod_pulses); False runs the messages in batch
        order without a workspace.

        ``sel_short`` / ``sel_long``: device int32 lists of the messages to run with the short /
        long variant (MC: ``sel_short`` only), as sdx_select_lines builds them; the other
        messages keep an empty OK descriptor.  Without them every message runs, routed by length.
        """
        out = self.first_pass(kind, bd, rec_cap, heap_cap, sel_short, sel_long, mn_elig, mn_method, workspace)
        rec_cap, heap_cap = out["rec_cap"], out["heap_cap"]
        desc, rec, heap = self.fetch(out)
        # re-runs on the GPU: grown output buffers / the long variant's larger per-message staging
        for attempt in range(4):
            st = desc["status"]
            redo = np.nonzero((st == ST_OVF_OUT) | (st == ST_OVF_TILE))[0].astype(np.int32)
            if not len(redo):
                break
            if attempt == 3:
                raise RuntimeError("result staging overflow persists (pathological message)")
            rec_cap, heap_cap = 2 * rec_cap + 64 * len(redo), 2 * heap_cap + 8192 * len(redo)
            out2 = self.rerun_overlay(kind, bd, redo, rec_cap, heap_cap, mn_elig=mn_elig, mn_method=mn_method)
            d2, r2, h2 = self.fetch(out2)
            # merge: re-based records appended after the first pass
            base_r, base_h = len(rec), len(heap)
            r2 = r2.copy()
            r2["payload_off"] += base_h
            rec = np.concatenate([rec, r2])
            heap = np.concatenate([heap, h2])
            for i in redo:
                d = d2[i].copy()
                d["rec_begin"] += base_r
                desc[i] = d
        return desc, rec, heap

    def first_pass(self, kind: int, bd, rec_cap: Optional[int] = None, heap_cap: Optional[int] = None,
                   sel_short=None, sel_long=None, mn_elig: int = 0, mn_method: int = -1, workspace: bool = True,
                   wire: bool = False):
        """Output buffers sized for a device batch (default capacities: 8 records and 200 payload
        bytes per message) and the first pass's launches into them (launch_routed), enqueued on the
        current stream; returns the output dict (run() re-runs what overflowed).  ``wire``: the
        kernels also write the exchange's counts (alloc_out), where every message of the launch goes
        to a kernel that writes them (k_pulses, k_mc: not MN, not MC batches with frames for the
        general MC kernel)."""
        n = bd["n"]
        selected = sel_short is not None or sel_long is not None
        if selected:
            n_work = sum(int(s.numel()) for s in (sel_short, sel_long) if s is not None)
        else:
            n_work = n
            lengths = bd["lengths"]
            if kind == KIND_MN:
                if n and int(lengths.max(initial=0)) > MN_HEX_MAX:
                    raise NotImplementedError(f"MN frames longer than {MN_HEX_MAX} hex characters are outside "
                                              "the device contract")
            elif kind == KIND_MC:
                pass   # frames longer than MC_HEX_MAX run on the general MC kernel (below)
            elif n and int(lengths.max(initial=0)) > LONG_MAX:
                raise NotImplementedError(f"messages longer than {LONG_MAX} pulses are outside the device contract")
        rec_cap = rec_cap or (8 * n_work + 1024)
        heap_cap = heap_cap or (200 * n_work + 65536)
        if kind == KIND_MN and not selected:   # parser mode: <= n_mn results of <= preamble + frame bytes
            rec_cap = max(rec_cap, 4 * n_work + 1024)
            heap_cap = max(heap_cap, int(4 * int(np.sum(bd["lengths"])) + 160 * n_work + 65536))
        if wire and (kind == KIND_MN or (kind == KIND_MC and not selected and bool((bd["lengths"] > MC_HEX_MAX).any()))):
            wire = False
        out = self.alloc_out(n, rec_cap, heap_cap,
                             self.pulses_work_bytes(n_work) if workspace and kind in (KIND_MU, KIND_MS) else 0, wire=wire)
        self.launch_routed(kind, bd, out, sel_short=sel_short, sel_long=sel_long, mn_elig=mn_elig, mn_method=mn_method,
                           workspace=workspace)
        return out

    def launch_routed(self, kind: int, bd, out, sel_short=None, sel_long=None, mn_elig: int = 0, mn_method: int = -1,
                      workspace: bool = True) -> None:
        """The first pass of run(): every message (or the given selection lists) to the launch that
        takes it -- MU/MS: the short variant (grouped order, spill regions) for <= SHORT_MAX pulses,
        the long one above; MC: k_mc, frames of more than MC_HEX_MAX characters on the general MC
        kernel; MN: k_mn.  Enqueued on the current stream, no host synchronisation."""
        t = self.torch
        if kind == KIND_MN:
            self.launch_mn(bd, out, elig=mn_elig, method=mn_method, sel=sel_short)
        elif sel_short is not None or sel_long is not None:
            if sel_short is not None and sel_short.numel():
                (self.launch_mc(bd, out, sel=sel_short) if kind == KIND_MC else
                 self.launch_pulses(kind, bd, out, sel=sel_short, group=workspace))
            if sel_long is not None and sel_long.numel():
                self.launch_pulses(kind, bd, out, sel=sel_long, long_variant=True)
        elif kind == KIND_MC:
            lengths = bd["lengths"]
            longf = lengths > MC_HEX_MAX
            if not longf.any():
                self.launch_mc(bd, out)
            else:   # k_mc takes <= MC_HEX_MAX characters; longer frames: sdx_demod_mc_general
                if not longf.all():
                    self.launch_mc(bd, out, sel=t.from_numpy(np.nonzero(~longf)[0].astype(np.int32)).to(self.dev))
                self.launch_mc_general(bd, out, t.from_numpy(np.nonzero(longf)[0].astype(np.int32)).to(self.dev),
                                       int(lengths.max()))
        else:
            lengths = bd["lengths"]
            short = lengths <= SHORT_MAX
            if short.all():
                self.launch_pulses(kind, bd, out, group=workspace)
            else:
                if short.any():
                    self.launch_pulses(kind, bd, out, sel=t.from_numpy(np.nonzero(short)[0].astype(np.int32)).to(self.dev),
                                       group=workspace)
                self.launch_pulses(kind, bd, out, sel=t.from_numpy(np.nonzero(~short)[0].astype(np.int32)).to(self.dev),
                                   long_variant=True)

    def overlay_out(self, n: int, rec_cap: int, heap_cap: int, wire: bool = False):
        """Output buffers of an exchange overlay (include/sdx.h ABI 11): every descriptor at
        ST_ABSENT until a launch writes it."""
        o = self.alloc_out(n, rec_cap, heap_cap, wire=wire)
        o["desc"].fill_(ST_ABSENT)
        return o

    def rerun_overlay(self, kind: int, bd, redo: np.ndarray, rec_cap: int, heap_cap: int, mn_elig: int = 0,
                      mn_method: int = -1):
        """Re-run the messages ``redo`` (host int array of batch indices whose first pass overflowed)
        into a fresh overlay: MU/MS on the long variant (larger per-message staging), MC on k_mc or,
        for frames of more than MC_HEX_MAX characters (k_mc hands them over as ST_OVF_TILE), on
        sdx_demod_mc_general, MN on k_mn; grown output capacities.  Enqueued on the current stream."""
        t = self.torch
        redo = np.asarray(redo, np.int32)
        # MU/MS re-run on the long k_pulses variant, which writes the exchange's counts (ABI 12)
        out2 = self.overlay_out(bd["n"], rec_cap, heap_cap, wire=kind in (KIND_MU, KIND_MS))
        sel = t.from_numpy(redo).to(self.dev)
        if kind == KIND_MN:
            self.launch_mn(bd, out2, elig=mn_elig, method=mn_method, sel=sel)
        elif kind == KIND_MC:
            if "lengths" in bd:
                rl = np.asarray(bd["lengths"])[redo]
            else:                # a line batch: the frames' lengths are on the device
                rl = bd["len"][t.from_numpy(redo.astype(np.int64)).to(self.dev)].cpu().numpy()
            lr = rl > MC_HEX_MAX
            if (~lr).any():
                self.launch_mc(bd, out2, sel=t.from_numpy(redo[~lr]).to(self.dev))
            if lr.any():
                self.launch_mc_general(bd, out2, t.from_numpy(redo[lr]).to(self.dev), int(rl.max()))
        else:
            self.launch_pulses(kind, bd, out2, sel=sel, long_variant=True)
        out2["_sel"] = sel          # alive until the launches have run
        return out2

    def merge_overlay(self, out, ov, redo: np.ndarray):
        """A launch's outputs and the overlay that re-ran its messages ``redo`` (rerun_overlay) as ONE
        output dict on the device, for what reads a launch through its descriptors (launch_json,
        mark_repeats): the overlay's records and payloads appended after the launch's, re-based as run()
        re-bases them on the host, and the descriptors of ``redo`` taken from the overlay.  Index
        plumbing of a rare path (one host read of the two cursors); the cursor's overflow word is the
        overlay's."""
        t = self.torch
        c0 = out["cursor"].cpu().numpy().astype(np.uint32)
        c1 = ov["cursor"].cpu().numpy().astype(np.uint32)
        r0, h0 = min(int(c0[0]), out["rec_cap"]), min(int(c0[1]), out["heap_cap"])
        r1, h1 = min(int(c1[0]), ov["rec_cap"]), min(int(c1[1]), ov["heap_cap"])
        rs = RES_DT.itemsize
        rec1 = ov["rec"][: r1 * rs].view(t.int32).view(-1, rs // 4).clone()
        rec1[:, 0] += h0                                   # sdx_result.payload_off
        idx = t.from_numpy(np.asarray(redo, np.int64)).to(self.dev)
        desc = out["desc"].clone()
        d0 = desc[: out["n"] * DESC_DT.itemsize].view(t.int32).view(-1, 2)
        d1 = ov["desc"][: out["n"] * DESC_DT.itemsize].view(t.int32).view(-1, 2)[idx].clone()
        d1[:, 0] += r0                                     # sdx_desc.rec_begin
        d0[idx] = d1
        # (one spare record / byte behind the declared capacities: never an empty buffer)
        return {"desc": desc, "rec": t.cat([out["rec"][: r0 * rs], rec1.view(-1).view(t.uint8), out["rec"][:rs]]),
                "heap": t.cat([out["heap"][:h0], ov["heap"][:h1], out["heap"][:1]]),
                "cursor": t.tensor([r0 + r1, h0 + h1, int(c1[2]), int(c0[3])], dtype=t.int32, device=self.dev),
                "work": None, "wire": None, "xrec": None, "rec_cap": r0 + r1, "heap_cap": h0 + h1, "n": out["n"]}

    def fetch(self, out):
        self.torch.cuda.current_stream(self.dev).synchronize()
        cur = out["cursor"].cpu().numpy().astype(np.uint32)
        n = out["n"]
        desc = out["desc"][: n * DESC_DT.itemsize].cpu().numpy().view(DESC_DT).copy()
        nrec = min(int(cur[0]), out["rec_cap"])
        nheap = min(int(cur[1]), out["heap_cap"])
        rec = out["rec"][: nrec * RES_DT.itemsize].cpu().numpy().view(RES_DT).copy()
        heap = out["heap"][:nheap].cpu().numpy().copy()
        return desc, rec, heap

    def format_floats(self, values, json_form: bool = False) -> "list[bytes]":
        """sdx_format_floats on this engine's device: repr(x) / json.dumps(x) of every double, as bytes."""
        return UnitRunner.get(self.device).format_floats(values, json_form)


# ---- unit-level entry (sdx_units) ----------------------------------------------------------------
UNIT_POSTDEMO, UNIT_HEX2BIN, UNIT_BIN2HEX, UNIT_MC2DMC, UNIT_PEXISTS, UNIT_MC_METHOD = 1, 2, 3, 4, 5, 6
UNIT_MC_BITS, UNIT_PX_SEARCH, UNIT_PX_PAT = 512, 32, 16

_UNIT_RUNNERS: Dict[int, "UnitRunner"] = {}


class UnitRunner:
    """sdx_units launches on one device (no bank needed: every input travels with the call)."""

    def __init__(self, device: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("pysignalduino_amd needs a ROCm GPU (MI355X); no CPU fallback exists")
        self.torch = torch
        self.lib = load_library()
        self.dev = torch.device("cuda", device)

    @staticmethod
    def get(device: int = 0) -> "UnitRunner":
        r = _UNIT_RUNNERS.get(device)
        if r is None:
            r = _UNIT_RUNNERS[device] = UnitRunner(device)
        return r

    def run(self, op: int, ins, caps, args=None, vals=None, mcrecs=None):
        """Run one op over the byte strings ``ins`` (``caps[i]``: payload capacity of item i).
        ``vals``: per-item float64 arrays (UNIT_PEXISTS); ``mcrecs``: numpy MC_REC array (UNIT_MC_METHOD).
        Returns (desc, rec, heap) as host numpy arrays, one desc/rec per item."""
        t, d = self.torch, self.dev
        n = len(ins)
        if n == 0:
            return np.zeros(0, DESC_DT), np.zeros(0, RES_DT), np.zeros(0, np.uint8)
        lens = np.fromiter((len(b) for b in ins), np.int64, n)
        in_off = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=in_off[1:])
        data = np.frombuffer(b"".join(ins) + b"\0" * 8, np.uint8)
        out_off = np.zeros(n + 1, np.int64)
        np.cumsum(np.asarray(caps, np.int64), out=out_off[1:])
        keep = []

        def dev(a):
            a = np.ascontiguousarray(a)
            if not a.flags.writeable:
                a = a.copy()
            x = t.from_numpy(a).to(d)
            keep.append(x)
            return _ptr(x)

        val_p = val_off_p = mc_p = None
        if vals is not None:
            vl = np.fromiter((len(v) for v in vals), np.int64, n)
            val_off = np.zeros(n + 1, np.int64)
            np.cumsum(vl, out=val_off[1:])
            flat = np.concatenate([np.asarray(v, np.float64) for v in vals] + [np.zeros(1)])
            val_p, val_off_p = dev(flat), dev(val_off)
        if mcrecs is not None:
            mc_p = dev(np.frombuffer(np.ascontiguousarray(mcrecs).tobytes(), np.uint8))
        heap_cap = int(out_off[-1])
        out = {"desc": t.zeros(n * DESC_DT.itemsize, dtype=t.uint8, device=d),
               "rec": t.zeros(n * RES_DT.itemsize, dtype=t.uint8, device=d),
               "heap": t.zeros(max(heap_cap, 1), dtype=t.uint8, device=d),
               "cursor": t.zeros(4, dtype=t.int32, device=d)}
        b = SdxUnitBatch(op, n, dev(data), dev(in_off), None if args is None else dev(np.asarray(args, np.int32)),
                         val_p, val_off_p, mc_p, dev(out_off))
        o = SdxOut(_ptr(out["desc"]), _ptr(out["rec"]), _ptr(out["heap"]), _ptr(out["cursor"]), n, max(heap_cap, 1), None, 0)
        _check(self.lib, self.lib.sdx_units(ctypes.byref(b), ctypes.byref(o),
                                            c_void_p(t.cuda.current_stream(d).cuda_stream)))
        t.cuda.current_stream(d).synchronize()
        desc = out["desc"].cpu().numpy().view(DESC_DT).copy()
        rec = out["rec"].cpu().numpy().view(RES_DT).copy()
        heap = out["heap"].cpu().numpy()
        return desc, rec, heap

    def parse_floats(self, strs: Sequence[bytes]):
        """sdx_parse_floats over the byte strings: (cls uint8[n], bits uint64[n]) as host numpy arrays."""
        t, d = self.torch, self.dev
        n = len(strs)
        if n == 0:
            return np.zeros(0, np.uint8), np.zeros(0, np.uint64)
        off = np.zeros(n + 1, np.int64)
        np.cumsum(np.fromiter((len(b) for b in strs), np.int64, n), out=off[1:])
        data = t.from_numpy(np.frombuffer(b"".join(strs) + b"\0" * 16, np.uint8).copy()).to(d)
        offs = t.from_numpy(off).to(d)
        val = t.empty(n, dtype=t.float64, device=d)
        cls = t.empty(n, dtype=t.uint8, device=d)
        b = SdxLines(_ptr(data), _ptr(offs), n)
        _check(self.lib, self.lib.sdx_parse_floats(ctypes.byref(b), _ptr(val), _ptr(cls),
                                                   c_void_p(t.cuda.current_stream(d).cuda_stream)))
        return cls.cpu().numpy(), val.cpu().numpy().view(np.uint64)

    def format_floats(self, values, json_form: bool = False) -> "list[bytes]":
        """sdx_format_floats over the doubles (a float64 array, or a uint64 array of bit patterns):
        repr(x), or json.dumps(x) with ``json_form``, of each as ASCII bytes."""
        t, d = self.torch, self.dev
        a = np.asarray(values)
        a = a.view(np.float64) if a.dtype == np.uint64 else a.astype(np.float64)
        a = np.ascontiguousarray(a).reshape(-1)
        n = len(a)
        if n == 0:
            return []
        val = t.from_numpy(a.view(np.int64).copy()).to(d)      # bit patterns: a nan keeps its payload
        text = t.empty(32 * n, dtype=t.uint8, device=d)
        _check(self.lib, self.lib.sdx_format_floats(_ptr(val), n, 1 if json_form else 0, _ptr(text),
                                                    c_void_p(t.cuda.current_stream(d).cuda_stream)))
        rows = text.cpu().numpy().reshape(n, 32)
        lens = rows[:, 31].tolist()
        if max(lens) > 24:
            raise RuntimeError("sdx_format_floats: a text longer than 24 bytes")
        flat = rows.tobytes()
        return [flat[32 * i: 32 * i + k] for i, k in enumerate(lens)]
