"""shafa-cd_amd — MI355X-native implementation of Shafa's block-codec hot path (Modules F, C, D).

This Python layer is plumbing only: it binds the C-ABI of ``libshafa_hip.so`` (include/shafa_hip.h)
with ctypes so that tests and bench.py can drive the HIP kernels with device memory owned by
PyTorch.  The product is the shared library (hand-written HIP for gfx950) and the C host in
``host/`` that mirrors the reference's module entry points.

The directory name contains a hyphen, so import it by path (tests/pkgload.py) — it registers
itself as ``shafa_cd_amd``.

There is NO CPU fallback: if the HIP library is missing, importing ``hip`` members raises.
"""
import collections
import ctypes as C
import itertools
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, "libshafa_hip.so")
HOST_LIB_PATH = os.path.join(PKG_DIR, "libshafa_host.so")
CLI_PATH = os.path.join(PKG_DIR, "bin", "shafa")

# _modules_error values (reference utils/errors.h:5-16) + device error
SUCCESS, OUTSIDE_MODULE, LACK_OF_MEMORY, FILE_INACCESSIBLE, FILE_UNRECOGNIZABLE = 0, 1, 2, 3, 4
FILE_STREAM_FAILED, FILE_TOO_SMALL, THREAD_CREATION_FAILED, THREAD_TERMINATION_FAILED = 5, 6, 7, 8
DEVICE_ERROR = 9
RLE_DECODE_MAX = 67108864 + 1024

BLOCK_SIZES = {"K": 655360, "m": 8388608, "M": 67108864, None: 65536}   # shafa.c:97-104,304-305


class CodeTable(C.Structure):
    """Binary form of one .cod block: len[s] bits, bits[s] MSB-first (include/shafa_hip.h)."""
    _fields_ = [("len", C.c_uint8 * 256), ("bits", (C.c_uint8 * 32) * 256)]

    def lens(self):
        return np.ctypeslib.as_array(self.len).copy()

    @classmethod
    def from_strings(cls, codes):
        """codes: 256 strings of '0'/'1' (the fields of a .cod block)."""
        t = cls()
        assert len(codes) == 256
        for s, code in enumerate(codes):
            t.len[s] = len(code)
            for i, ch in enumerate(code):
                if ch == "1":
                    t.bits[s][i >> 3] |= 0x80 >> (i & 7)
        return t


class PipeResult(C.Structure):
    """shafa_pipe_result (include/shafa_hip.h, layer 3)."""
    _fields_ = [("out", C.c_void_p), ("out_n", C.c_size_t), ("mid_n", C.c_size_t),
                ("freq", C.c_uint64 * 256), ("freq_in", C.c_uint64 * 256)]


class PipeBlock(C.Structure):
    """shafa_pipe_block (include/shafa_hip.h, layer 3 groups)."""
    _fields_ = [("in_off", C.c_size_t), ("in_n", C.c_size_t), ("table", C.POINTER(CodeTable)), ("n_symbols", C.c_size_t),
                ("out_cap", C.c_size_t)]


PIPE_GROUP_MAX = 256
OP_HIST, OP_RLE_ENCODE, OP_SF_ENCODE, OP_SF_DECODE, OP_RLE_DECODE, OP_SF_RLE_DECODE, OP_FTC = 1, 2, 3, 4, 5, 6, 7
PIPE_INPUT_HIST, PIPE_FTC_RLE, PIPE_FTC_PLAIN = 1, 2, 4


class ShafaError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__(f"shafa_hip error {code} {what}")


_lib = None


def lib():
    """Load libshafa_hip.so (built by __graft_entry__.build()).  Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    u8p, u64p, szp, vp = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t), C.c_void_p
    tp = C.POINTER(CodeTable)
    L.shafa_hip_abi_version.restype = C.c_int
    L.shafa_hip_device_count.restype = C.c_int
    L.shafa_hip_init.argtypes = [C.c_int]
    L.shafa_hip_last_error.restype = C.c_char_p
    L.shafa_hip_set_option.argtypes = [C.c_char_p, C.c_long]
    L.shafa_hip_set_option.restype = C.c_int
    L.shafa_hip_hist256.argtypes = [u8p, C.c_size_t, u64p]
    L.shafa_hip_rle_encode.argtypes = [u8p, C.c_size_t, u8p, C.c_size_t, szp, u64p]
    L.shafa_hip_sf_encode.argtypes = [u8p, C.c_size_t, tp, u8p, C.c_size_t, szp]
    L.shafa_hip_sf_decode.argtypes = [u8p, C.c_size_t, tp, u8p, C.c_size_t]
    L.shafa_hip_rle_decode.argtypes = [u8p, C.c_size_t, u8p, C.c_size_t, szp]
    L.shafa_hipd_batch_create.argtypes = [C.c_int, C.c_size_t, C.POINTER(vp)]
    L.shafa_hipd_batch_destroy.argtypes = [vp]
    L.shafa_hipd_batch_destroy.restype = None
    L.shafa_hipd_hist256.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp]
    L.shafa_hipd_rle_encode.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, u8p, u64p, u64p, vp, vp]
    L.shafa_hipd_sf_encode.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, tp, u8p, u64p, u64p, vp]
    L.shafa_hipd_sf_decode.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, tp, u64p, u8p, u64p]
    L.shafa_hipd_rle_decode.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, u8p, u64p, u64p, vp]
    L.shafa_hipd_sf_build_codes.argtypes = [vp, vp, C.c_int, vp, vp]
    L.shafa_hip_tile_hist_bytes.argtypes = [C.c_size_t]
    L.shafa_hip_tile_hist_bytes.restype = C.c_size_t
    L.shafa_hipd_hist256_tiles.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_rle_encode_tiles.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, u8p, u64p, u64p, vp, vp, u8p, u64p]
    L.shafa_hipd_sf_encode_tiles.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, tp, u8p, u64p, u8p, u64p, u64p, vp]
    L.shafa_hipd_sf_encode_dev.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp, vp, u8p, u64p, u8p, u64p, u64p, vp]
    L.shafa_hipd_sf_decode_dev.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp, vp, vp, u8p, u64p, u64p]
    L.shafa_hipd_rle_decode_dev.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp, u8p, u64p, u64p, vp]
    L.shafa_hipd_rle_decoded_size_dev.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp, vp]
    L.shafa_hipd_rle_encoded_size_dev.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp, vp]
    L.shafa_hipd_rle_encoded_hist_dev.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp, vp, vp]
    L.shafa_hipd_sf_encoded_size_dev.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    L.shafa_hipd_compare_dev.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp, u8p, u64p, u64p, vp]
    L.shafa_hipd_crc32_dev.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp, vp]
    L.shafa_hipd_crc32_combine_dev.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), vp, vp, vp, vp]
    L.shafa_hipd_find_dev.argtypes = [vp, vp, C.c_int, u8p, u64p, u64p, vp, C.c_char_p, u64p, C.c_char_p, C.c_uint32, C.c_uint64,
                                      vp, vp, vp]
    L.shafa_hipd_split_planes_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_merge_planes_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_split_records_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_merge_records_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_split_planes_diff_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_merge_planes_diff_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_split_planes_lag_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u64p, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_merge_planes_lag_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u64p, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_split_planes_grid_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, u64p, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_merge_planes_grid_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, u64p, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_hist_planes_grid_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, u64p, u8p, u64p, u64p, vp, vp]
    f64p = C.POINTER(C.c_double)
    L.shafa_hipd_split_planes_grid_quant_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, u64p, f64p, f64p, u8p, u64p, u64p,
                                                         vp, u8p, u64p, vp, u64p, u64p, vp]
    L.shafa_hipd_merge_planes_grid_quant_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, u64p, f64p, u8p, u64p, u64p, vp,
                                                         vp, u64p, u64p, u8p, u64p]
    L.shafa_hipd_hist_planes_grid_quant_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, u64p, f64p, f64p, u8p, u64p, u64p,
                                                        vp, vp, vp]
    u32p = C.POINTER(C.c_uint32)
    L.shafa_hipd_split_planes_grid_round_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, u64p, u32p, u32p, u8p, u64p, u64p,
                                                         vp, u8p, u64p, vp, u64p, u64p, vp]
    L.shafa_hipd_merge_planes_grid_round_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, u64p, u32p, u32p, u8p, u64p, u64p,
                                                         vp, vp, u64p, u64p, u8p, u64p]
    L.shafa_hipd_hist_planes_grid_round_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, u64p, u32p, u32p, u8p, u64p, u64p,
                                                        vp, vp, vp]
    L.shafa_hipd_error_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u32p, f64p, f64p, u8p, u64p, u64p, vp, u8p, u64p, vp]
    L.shafa_hipd_error_quant_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, f64p, f64p, u8p, u64p, u64p, vp, vp]
    L.shafa_hipd_error_round_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u32p, u32p, u8p, u64p, u64p, vp, vp]
    L.shafa_hipd_split_planes_xor_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u8p, u64p, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_merge_planes_xor_dev.argtypes = [vp, vp, C.c_int, C.c_uint32, u8p, u64p, u8p, u64p, u64p, vp, u8p, u64p]
    L.shafa_hipd_seek_index_dev.argtypes =[vp, vp, C.c_int, u8p, u64p, u64p, vp, vp, C.c_uint32, C.c_int, u64p, vp, vp, vp]
    L.shafa_hipd_read_spans_dev.argtypes = [vp, vp, C.c_int, u8p, C.c_uint64, u64p, u64p, u64p, u64p, vp, C.c_uint32, C.c_int, vp,
                                            C.c_int, C.POINTER(C.c_int), u64p, u64p, u64p, u64p, u64p, u8p, C.c_uint64]
    L.shafa_hipd_finish.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.shafa_hip_pack_payloads_max.argtypes = [C.c_int, u64p, C.c_int]
    L.shafa_hip_pack_payloads_max.restype = C.c_size_t
    L.shafa_hip_pack_cod_max.argtypes = [C.c_int]
    L.shafa_hip_pack_cod_max.restype = C.c_size_t
    L.shafa_hip_pack_freq_max.argtypes = [C.c_int]
    L.shafa_hip_pack_freq_max.restype = C.c_size_t
    L.shafa_hipd_pack_payloads.argtypes = [vp, vp, C.c_int, C.c_int, u8p, u64p, u64p, vp, u8p, C.c_uint64, vp]
    L.shafa_hipd_pack_cod.argtypes = [vp, vp, C.c_int, C.c_char, vp, vp, u8p, C.c_uint64, vp]
    L.shafa_hipd_pack_freq.argtypes = [vp, vp, C.c_int, C.c_char, vp, vp, u8p, C.c_uint64, vp]
    i32p = C.POINTER(C.c_int)
    L.shafa_hipd_pack_payloads_files.argtypes = [vp, vp, C.c_int, i32p, i32p, C.c_int, u8p, u64p, u64p, vp, u8p, u64p, u64p,
                                                 vp]
    L.shafa_hipd_pack_cod_files.argtypes = [vp, vp, C.c_int, i32p, i32p, C.c_char_p, vp, vp, u8p, u64p, u64p, vp]
    L.shafa_hipd_pack_freq_files.argtypes = [vp, vp, C.c_int, i32p, i32p, C.c_char_p, vp, vp, u8p, u64p, u64p, vp]
    L.shafa_hipd_unpack_cod.argtypes = [vp, vp, C.c_int, u8p, C.c_uint64, vp, vp, vp]
    L.shafa_hipd_unpack_rle_freq.argtypes = [vp, vp, C.c_int, u8p, C.c_uint64, C.c_uint64, vp, vp, vp]
    L.shafa_hipd_unpack_freq.argtypes = [vp, vp, C.c_int, u8p, C.c_uint64, vp, vp, vp]
    L.shafa_hipd_unpack_shaf.argtypes = [vp, vp, C.c_int, u8p, C.c_uint64, vp, vp, vp]
    L.shafa_hipd_unpack_payloads.argtypes = [vp, vp, C.c_int, u8p, C.c_uint64, vp, vp, u8p, u64p, u64p]
    L.shafa_hipd_unpack_cod_files.argtypes = [vp, vp, C.c_int, i32p, i32p, u8p, u64p, u64p, vp, vp, vp]
    L.shafa_hipd_unpack_rle_freq_files.argtypes = [vp, vp, C.c_int, i32p, i32p, u8p, u64p, u64p, u64p, u64p, vp, vp, vp]
    L.shafa_hipd_unpack_shaf_files.argtypes = [vp, vp, C.c_int, i32p, i32p, u8p, u64p, u64p, vp, vp, vp]
    L.shafa_hipd_gen_bytes.argtypes = [vp, C.c_uint64, C.c_uint64, u8p, u8p, C.c_size_t]
    L.shafa_pipe_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.shafa_pipe_destroy.argtypes = [vp]
    L.shafa_pipe_destroy.restype = None
    L.shafa_pipe_slots.argtypes = [vp]
    L.shafa_pipe_slot_device.argtypes = [vp, C.c_int]
    L.shafa_pipe_slot_device.restype = C.c_int
    L.shafa_hip_init_devices.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.shafa_hip_init_devices.restype = C.c_int
    L.shafa_hip_devices.restype = C.c_int
    L.shafa_pipe_in.argtypes = [vp, C.c_int, C.c_size_t]
    L.shafa_pipe_in.restype = C.c_void_p
    L.shafa_pipe_submit.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, tp, C.c_size_t, C.c_size_t, C.c_int]
    L.shafa_pipe_wait.argtypes = [vp, C.c_int, C.POINTER(PipeResult)]
    L.shafa_pipe_submit_group.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(PipeBlock), C.c_int]
    L.shafa_pipe_wait_group.argtypes = [vp, C.c_int, C.c_int, C.POINTER(PipeResult), C.POINTER(C.c_int)]
    L.shafa_pipe_ftc_encode.argtypes = [vp, C.c_int, C.c_int, tp, C.c_size_t]
    for name in ("shafa_pipe_create", "shafa_pipe_slots", "shafa_pipe_submit", "shafa_pipe_wait", "shafa_pipe_submit_group",
                 "shafa_pipe_wait_group", "shafa_pipe_ftc_encode"):
        getattr(L, name).restype = C.c_int
    for name in ("shafa_hip_init", "shafa_hip_hist256", "shafa_hip_rle_encode", "shafa_hip_sf_encode",
                 "shafa_hip_sf_decode", "shafa_hip_rle_decode", "shafa_hipd_batch_create",
                 "shafa_hipd_hist256", "shafa_hipd_rle_encode", "shafa_hipd_sf_encode",
                 "shafa_hipd_sf_decode", "shafa_hipd_rle_decode", "shafa_hipd_finish",
                 "shafa_hipd_gen_bytes", "shafa_hipd_hist256_tiles", "shafa_hipd_rle_encode_tiles",
                 "shafa_hipd_sf_encode_tiles", "shafa_hipd_sf_encode_dev", "shafa_hipd_sf_decode_dev",
                 "shafa_hipd_rle_decode_dev", "shafa_hipd_pack_payloads", "shafa_hipd_pack_cod", "shafa_hipd_pack_freq",
                 "shafa_hipd_pack_payloads_files", "shafa_hipd_pack_cod_files", "shafa_hipd_pack_freq_files",
                 "shafa_hipd_unpack_cod", "shafa_hipd_unpack_rle_freq", "shafa_hipd_unpack_shaf", "shafa_hipd_unpack_payloads",
                 "shafa_hipd_unpack_cod_files", "shafa_hipd_unpack_rle_freq_files", "shafa_hipd_unpack_shaf_files",
                 "shafa_hipd_rle_decoded_size_dev", "shafa_hipd_rle_encoded_size_dev", "shafa_hipd_rle_encoded_hist_dev",
                 "shafa_hipd_sf_encoded_size_dev", "shafa_hipd_unpack_freq", "shafa_hipd_compare_dev", "shafa_hipd_crc32_dev",
                 "shafa_hipd_crc32_combine_dev", "shafa_hipd_seek_index_dev", "shafa_hipd_read_spans_dev",
                 "shafa_hipd_find_dev", "shafa_hipd_split_planes_dev", "shafa_hipd_merge_planes_dev",
                 "shafa_hipd_split_planes_xor_dev", "shafa_hipd_merge_planes_xor_dev",
                 "shafa_hipd_split_planes_diff_dev", "shafa_hipd_merge_planes_diff_dev",
                 "shafa_hipd_split_planes_lag_dev", "shafa_hipd_merge_planes_lag_dev",
                 "shafa_hipd_split_planes_grid_dev", "shafa_hipd_merge_planes_grid_dev", "shafa_hipd_hist_planes_grid_dev",
                 "shafa_hipd_split_planes_grid_quant_dev", "shafa_hipd_merge_planes_grid_quant_dev",
                 "shafa_hipd_hist_planes_grid_quant_dev", "shafa_hipd_split_planes_grid_round_dev",
                 "shafa_hipd_merge_planes_grid_round_dev", "shafa_hipd_hist_planes_grid_round_dev",
                 "shafa_hipd_error_dev", "shafa_hipd_error_quant_dev", "shafa_hipd_error_round_dev",
                 "shafa_hipd_split_records_dev", "shafa_hipd_merge_records_dev"):
        getattr(L, name).restype = C.c_int
    _lib = L
    return L


def init_devices(devices=None):
    """Select the GPUs of the layer-3 pipeline (None: every visible device); include/shafa_hip.h: shafa_hip_init_devices."""
    if devices:
        arr = (C.c_int * len(devices))(*devices)
        _check(lib().shafa_hip_init_devices(arr, len(devices)), "init_devices")
    else:
        _check(lib().shafa_hip_init_devices(None, 0), "init_devices")
    return lib().shafa_hip_devices()


def set_option(name, value):
    """Tuning knobs of the library (include/shafa_hip.h: shafa_hip_set_option)."""
    _check(lib().shafa_hip_set_option(name.encode(), int(value)), "set_option " + name)


def _check(rc, what=""):
    if rc != SUCCESS:
        msg = lib().shafa_hip_last_error().decode() if rc == DEVICE_ERROR else ""
        raise ShafaError(rc, f"{what} {msg}")


def _np_u8(data):
    a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data
    return np.ascontiguousarray(a, dtype=np.uint8)


# ------------------------------------------------------------------ layer 1: host buffers, one block
def hist256(data):
    a = _np_u8(data)
    f = np.zeros(256, dtype=np.uint64)
    _check(lib().shafa_hip_hist256(a.ctypes.data, a.size, f.ctypes.data_as(C.POINTER(C.c_uint64))), "hist256")
    return f


def rle_encode(data, want_freq=False):
    a = _np_u8(data)
    out = np.empty(2 * a.size + 3, dtype=np.uint8)
    n = C.c_size_t(0)
    f = np.zeros(256, dtype=np.uint64) if want_freq else None
    fp = f.ctypes.data_as(C.POINTER(C.c_uint64)) if want_freq else None
    _check(lib().shafa_hip_rle_encode(a.ctypes.data, a.size, out.ctypes.data, out.size, C.byref(n), fp), "rle_encode")
    return (out[:n.value].copy(), f) if want_freq else out[:n.value].copy()


def sf_encode(data, table, cap=None, raw_rc=False):
    a = _np_u8(data)
    cap = cap if cap is not None else a.size * 32 + 16
    out = np.empty(max(cap, 1), dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().shafa_hip_sf_encode(a.ctypes.data, a.size, C.byref(table), out.ctypes.data, cap, C.byref(n))
    if raw_rc:
        return rc, out[:n.value].copy()
    _check(rc, "sf_encode")
    return out[:n.value].copy()


def sf_decode(data, table, n_symbols, raw_rc=False):
    a = _np_u8(data)
    out = np.empty(max(n_symbols, 1), dtype=np.uint8)
    rc = lib().shafa_hip_sf_decode(a.ctypes.data, a.size, C.byref(table), out.ctypes.data, n_symbols)
    if raw_rc:
        return rc, out[:n_symbols].copy()
    _check(rc, "sf_decode")
    return out[:n_symbols].copy()


def rle_decode(data, cap=None, raw_rc=False):
    a = _np_u8(data)
    cap = cap if cap is not None else min(a.size * 255 + 16, RLE_DECODE_MAX)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().shafa_hip_rle_decode(a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(n))
    if raw_rc:
        return rc, out[:n.value].copy()
    _check(rc, "rle_decode")
    return out[:n.value].copy()


# ------------------------------------------------------------------ layer 2: device buffers, batches
def _u64arr(v):
    return np.ascontiguousarray(v, dtype=np.uint64)


def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _f64arr(v):
    return np.ascontiguousarray(v, dtype=np.float64)


def _pf64(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _u32arr(v):
    return np.ascontiguousarray(v, dtype=np.uint32)


def _pu32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _grid_lags(what, lags, nblocks):
    """the lags of a _grid launch, one tuple per block -> (nlags, the uint64 array [nblocks * nlags]), every tuple padded with 0
    to the call's widest (what the entry makes of the values is the entry's to say)"""
    rows = [tuple(int(g) for g in row) for row in lags]
    if len(rows) != nblocks:
        raise ValueError(f"{what}: one tuple of lags per block")
    nl = max([len(r) for r in rows] + [1])
    return nl, _u64arr([g for r in rows for g in r + (0,) * (nl - len(r))])


def _i32arr(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _ptr(t):
    """a tensor's address, None for an empty one (a file of 0 bytes may have no storage)"""
    return t.data_ptr() if t.numel() else None


def _addr(t):
    """a device address: a tensor's, or an int as it is (None for 0)"""
    return (t or None) if isinstance(t, int) else t.data_ptr()


class Batch:
    """Reusable batch context (shafa_hipd_batch).  Tensors are torch uint8/int64 CUDA tensors; the
    stream is a torch.cuda.Stream (or None for the library's own stream)."""

    def __init__(self, max_blocks, max_block_bytes):
        self.h = C.c_void_p()
        self.max_blocks = max_blocks
        _check(lib().shafa_hipd_batch_create(max_blocks, max_block_bytes, C.byref(self.h)), "batch_create")

    def close(self):
        if self.h:
            lib().shafa_hipd_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _st(stream):
        """hipStream_t of a torch stream.  The tensors handed to a launch were typically produced (allocated,
        filled, copied) by torch on ITS current stream: order this launch after that work."""
        if stream is None:
            return None
        import torch
        cur = torch.cuda.current_stream(stream.device)
        if cur.cuda_stream != stream.cuda_stream:
            stream.wait_stream(cur)
        return C.c_void_p(stream.cuda_stream)

    @staticmethod
    def _tables(tables):
        arr = (CodeTable * len(tables))()
        for i, t in enumerate(tables):
            C.memmove(C.byref(arr[i]), C.byref(t), C.sizeof(CodeTable))
        return arr

    # Every *_off / *_n / *_cap argument is a host sequence with one entry per block.
    def hist256(self, stream, d_in, in_off, in_n, d_freq):
        io, il = _u64arr(in_off), _u64arr(in_n)
        _check(lib().shafa_hipd_hist256(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(il),
                                        d_freq.data_ptr()), "hipd_hist256")

    def sf_build_codes(self, stream, nblocks, d_freq, d_tables):
        """Module T on the device: d_freq nblocks x 256 u64 -> d_tables nblocks x sizeof(CodeTable) bytes (device memory)."""
        _check(lib().shafa_hipd_sf_build_codes(self.h, self._st(stream), nblocks, d_freq.data_ptr(), d_tables.data_ptr()),
               "hipd_sf_build_codes")

    def rle_encode(self, stream, d_in, in_off, in_n, d_out, out_off, out_cap, d_out_n, d_freq=None):
        io, il, oo, oc = _u64arr(in_off), _u64arr(in_n), _u64arr(out_off), _u64arr(out_cap)
        _check(lib().shafa_hipd_rle_encode(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(il),
                                           d_out.data_ptr(), _p64(oo), _p64(oc), d_out_n.data_ptr(),
                                           d_freq.data_ptr() if d_freq is not None else None), "hipd_rle_encode")

    def sf_encode(self, stream, d_in, in_off, in_n, tables, d_out, out_off, out_cap, d_out_n):
        io, il, oo, oc = _u64arr(in_off), _u64arr(in_n), _u64arr(out_off), _u64arr(out_cap)
        tarr = tables if isinstance(tables, C.Array) else self._tables(tables)
        _check(lib().shafa_hipd_sf_encode(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(il),
                                          tarr, d_out.data_ptr(), _p64(oo), _p64(oc), d_out_n.data_ptr()),
               "hipd_sf_encode")

    # ---- with tile histograms (include/shafa_hip.h: "Tile histograms"): block b's at d_thist + thist_off[b] ----
    def hist256_tiles(self, stream, d_in, in_off, in_n, d_freq, d_thist, thist_off):
        io, il, to = _u64arr(in_off), _u64arr(in_n), _u64arr(thist_off)
        _check(lib().shafa_hipd_hist256_tiles(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(il),
                                              d_freq.data_ptr(), d_thist.data_ptr(), _p64(to)), "hipd_hist256_tiles")

    def rle_encode_tiles(self, stream, d_in, in_off, in_n, d_out, out_off, out_cap, d_out_n, d_freq, d_thist, thist_off):
        io, il, oo, oc, to = _u64arr(in_off), _u64arr(in_n), _u64arr(out_off), _u64arr(out_cap), _u64arr(thist_off)
        _check(lib().shafa_hipd_rle_encode_tiles(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(il),
                                                 d_out.data_ptr(), _p64(oo), _p64(oc), d_out_n.data_ptr(), d_freq.data_ptr(),
                                                 d_thist.data_ptr(), _p64(to)), "hipd_rle_encode_tiles")

    def sf_encode_tiles(self, stream, d_in, in_off, in_n, tables, d_thist, thist_off, d_out, out_off, out_cap, d_out_n):
        io, il, oo, oc, to = _u64arr(in_off), _u64arr(in_n), _u64arr(out_off), _u64arr(out_cap), _u64arr(thist_off)
        tarr = tables if isinstance(tables, C.Array) else self._tables(tables)
        _check(lib().shafa_hipd_sf_encode_tiles(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(il),
                                                tarr, d_thist.data_ptr(), _p64(to), d_out.data_ptr(), _p64(oo), _p64(oc),
                                                d_out_n.data_ptr()), "hipd_sf_encode_tiles")

    def sf_encode_dev(self, stream, d_in, in_off, in_cap, d_in_n, d_tables, d_out, out_off, out_cap, d_out_n,
                      d_thist=None, thist_off=None):
        """sf_encode[_tiles] with the block sizes (d_in_n: nblocks int64) and the code tables (d_tables: nblocks x
        sizeof(CodeTable) bytes, e.g. sf_build_codes' output) in device memory; in_cap bounds each block's size.  Enqueues
        only: nothing is read back (include/shafa_hip.h: shafa_hipd_sf_encode_dev)."""
        io, ic, oo, oc = _u64arr(in_off), _u64arr(in_cap), _u64arr(out_off), _u64arr(out_cap)
        to = _u64arr(thist_off) if thist_off is not None else None
        _check(lib().shafa_hipd_sf_encode_dev(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(ic),
                                              d_in_n.data_ptr(), d_tables.data_ptr(),
                                              d_thist.data_ptr() if d_thist is not None else None,
                                              _p64(to) if to is not None else None, d_out.data_ptr(), _p64(oo), _p64(oc),
                                              d_out_n.data_ptr()), "hipd_sf_encode_dev")

    def sf_decode_dev(self, stream, d_in, in_off, in_cap, d_in_n, d_tables, d_n_symbols, d_out, out_off, out_cap):
        """sf_decode with the stream sizes (d_in_n), the symbol counts (d_n_symbols: nblocks int64 each) and the code tables
        (d_tables: nblocks x sizeof(CodeTable) bytes, e.g. sf_build_codes' output) in device memory; in_cap / out_cap bound
        each block's regions.  Enqueues only: nothing is read back (include/shafa_hip.h: shafa_hipd_sf_decode_dev)."""
        io, ic, oo, oc = _u64arr(in_off), _u64arr(in_cap), _u64arr(out_off), _u64arr(out_cap)
        _check(lib().shafa_hipd_sf_decode_dev(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(ic),
                                              d_in_n.data_ptr(), d_tables.data_ptr(), d_n_symbols.data_ptr(),
                                              d_out.data_ptr(), _p64(oo), _p64(oc)), "hipd_sf_decode_dev")

    def rle_decode_dev(self, stream, d_in, in_off, in_cap, d_in_n, d_out, out_off, out_cap, d_out_n):
        """rle_decode with the block sizes (d_in_n: nblocks int64) in device memory; in_cap bounds each block's size.
        Enqueues only (include/shafa_hip.h: shafa_hipd_rle_decode_dev)."""
        io, ic, oo, oc = _u64arr(in_off), _u64arr(in_cap), _u64arr(out_off), _u64arr(out_cap)
        _check(lib().shafa_hipd_rle_decode_dev(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(ic),
                                               d_in_n.data_ptr(), d_out.data_ptr(), _p64(oo), _p64(oc),
                                               d_out_n.data_ptr()), "hipd_rle_decode_dev")

    def rle_decoded_size_dev(self, stream, d_in, in_off, in_cap, d_in_n, d_out_n):
        """d_out_n[b] (int64) = the size rle_decode_dev would leave for block b with out_cap = RLE_DECODE_MAX; nothing is
        decoded and no output exists.  Enqueues only (include/shafa_hip.h: shafa_hipd_rle_decoded_size_dev)."""
        io, ic = _u64arr(in_off), _u64arr(in_cap)
        _check(lib().shafa_hipd_rle_decoded_size_dev(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(ic),
                                                     d_in_n.data_ptr(), d_out_n.data_ptr()), "hipd_rle_decoded_size_dev")

    def rle_encoded_size_dev(self, stream, d_in, in_off, in_cap, d_in_n, d_out_n):
        """d_out_n[b] (int64) = the size rle_encode would leave for the d_in_n[b] bytes of block b with room enough; nothing
        is encoded and no output exists.  Enqueues only (include/shafa_hip.h: shafa_hipd_rle_encoded_size_dev)."""
        io, ic = _u64arr(in_off), _u64arr(in_cap)
        _check(lib().shafa_hipd_rle_encoded_size_dev(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(ic),
                                                     d_in_n.data_ptr(), d_out_n.data_ptr()), "hipd_rle_encoded_size_dev")

    def rle_encoded_hist_dev(self, stream, d_in, in_off, in_cap, d_in_n, d_out_n, d_freq):
        """d_freq[b * 256 + s] (int64) = the histogram rle_encode would leave for the d_in_n[b] bytes of block b with room
        enough, d_out_n[b] its size; nothing is encoded and no output exists.  d_freq is overwritten.  Enqueues only
        (include/shafa_hip.h: shafa_hipd_rle_encoded_hist_dev)."""
        io, ic = _u64arr(in_off), _u64arr(in_cap)
        _check(lib().shafa_hipd_rle_encoded_hist_dev(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(ic),
                                                     d_in_n.data_ptr(), d_out_n.data_ptr(), d_freq.data_ptr()),
               "hipd_rle_encoded_hist_dev")

    def sf_encoded_size_dev(self, stream, nblocks, d_freq, d_tables, d_out_n):
        """d_out_n[b] (int64) = the size sf_encode_dev would leave for a block with histogram d_freq[b * 256 ..] and table
        d_tables[b] with room enough; nothing is encoded.  Enqueues only (include/shafa_hip.h:
        shafa_hipd_sf_encoded_size_dev)."""
        _check(lib().shafa_hipd_sf_encoded_size_dev(self.h, self._st(stream), nblocks, d_freq.data_ptr(), d_tables.data_ptr(),
                                                    d_out_n.data_ptr()), "hipd_sf_encoded_size_dev")

    def compare_dev(self, stream, d_a, a_off, a_cap, d_a_n, d_ref, ref_off, ref_n, d_first):
        """d_first[b] (int64) = where the d_a_n[b] (int64, device; <= a_cap[b]) bytes of a decoder's region d_a + a_off[b]
        first differ from the ref_n[b] bytes at d_ref + ref_off[b] (any alignment, read in place), or the smaller of the two
        sizes.  A difference sets no error word.  Enqueues only (include/shafa_hip.h: shafa_hipd_compare_dev)."""
        ao, ac, ro, rn = _u64arr(a_off), _u64arr(a_cap), _u64arr(ref_off), _u64arr(ref_n)
        _check(lib().shafa_hipd_compare_dev(self.h, self._st(stream), len(ao), d_a.data_ptr(), _p64(ao), _p64(ac),
                                            d_a_n.data_ptr(), d_ref.data_ptr(), _p64(ro), _p64(rn), d_first.data_ptr()),
               "hipd_compare_dev")

    def crc32_dev(self, stream, d_in, in_off, in_cap, d_in_n, d_crc):
        """d_crc[b] (int32, the CRC's 32 bits) = zlib.crc32 of the d_in_n[b] (int64, device; <= in_cap[b]) bytes at
        d_in + in_off[b] (any alignment, read in place).  Enqueues only (include/shafa_hip.h: shafa_hipd_crc32_dev)."""
        io, ic = _u64arr(in_off), _u64arr(in_cap)
        _check(lib().shafa_hipd_crc32_dev(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(ic),
                                          d_in_n.data_ptr(), d_crc.data_ptr()), "hipd_crc32_dev")

    def crc32_combine_dev(self, stream, first, count, d_crc, d_n, d_file_crc, d_file_n):
        """file f = blocks first[f] .. first[f] + count[f] - 1 of d_crc (int32) / d_n (int64): d_file_crc[f] (int32) = the
        CRC-32 of their concatenation, d_file_n[f] (int64) its length, from the blocks' CRCs and lengths alone.  Enqueues only
        (include/shafa_hip.h: shafa_hipd_crc32_combine_dev)."""
        fi, co = _i32arr(first), _i32arr(count)
        _check(lib().shafa_hipd_crc32_combine_dev(self.h, self._st(stream), len(fi), _p32(fi), _p32(co), d_crc.data_ptr(),
                                                  d_n.data_ptr(), d_file_crc.data_ptr(), d_file_n.data_ptr()),
               "hipd_crc32_combine_dev")

    def find_dev(self, stream, d_in, in_off, in_cap, d_in_n, flags, pos, pattern, max_hits, d_hits, d_count, d_total):
        """The positions of `pattern` (1 .. 256 bytes) in the d_in_n[b] (int64, device; <= in_cap[b]) bytes at d_in + in_off[b]
        (any alignment, read in place), as pos[b] + the offset in the region: appended to d_hits (int64; None iff max_hits is 0)
        from index d_total[0] (int64, device) on while the index is below max_hits; d_count[b] (int64) = region b's matches,
        d_total[0] += their sum.  flags (None = all 0): FIND_NEXT = region b + 1 continues region b's stream, FIND_CONTEXT =
        matches that start in region b are not reported.  Enqueues only (include/shafa_hip.h: shafa_hipd_find_dev)."""
        io, ic, po = _u64arr(in_off), _u64arr(in_cap), _u64arr(pos)
        fl = None if flags is None else bytes(bytearray(flags))
        pat = bytes(pattern)
        _check(lib().shafa_hipd_find_dev(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(ic), d_in_n.data_ptr(),
                                         fl, _p64(po), pat, len(pat), int(max_hits), None if d_hits is None else d_hits.data_ptr(),
                                         d_count.data_ptr(), d_total.data_ptr()), "hipd_find_dev")

    def split_planes_dev(self, stream, elem, d_in, in_off, cap, d_n, d_planes, plane_off):
        """Block b's d_n[b] (int64, device; <= cap[b]) elements of `elem` = 1, 2, 4 or 8 bytes at d_in + in_off[b] (bytes, any
        alignment, read in place) -> their byte planes: plane j (byte j of every element, plane 0 the least significant) is
        d_n[b] bytes at d_planes + plane_off[b * elem + j].  d_planes and every plane offset are multiples of 16; nothing behind
        a plane's d_n[b] bytes is written.  d_in and d_planes are tensors or device addresses (int: the base that offsets into
        several tensors are measured from).  Enqueues only (include/shafa_hip.h: "Byte planes")."""
        io, ic, po = _u64arr(in_off), _u64arr(cap), _u64arr(plane_off)
        _check(lib().shafa_hipd_split_planes_dev(self.h, self._st(stream), len(io), elem, _addr(d_in), _p64(io), _p64(ic),
                                                 d_n.data_ptr(), _addr(d_planes), _p64(po)), "hipd_split_planes_dev")

    def merge_planes_dev(self, stream, elem, d_planes, plane_off, cap, d_n, d_out, out_off):
        """split_planes_dev's inverse: block b's planes (d_n[b] bytes each at d_planes + plane_off[b * elem + j], multiples of
        16) -> its elem * d_n[b] bytes at d_out + out_off[b] (any alignment); no other byte of d_out is written, the up to 15
        bytes on either side of an unaligned region included.  d_planes and d_out are tensors or device addresses (int).
        Enqueues only (include/shafa_hip.h: "Byte planes")."""
        po, ic, oo = _u64arr(plane_off), _u64arr(cap), _u64arr(out_off)
        _check(lib().shafa_hipd_merge_planes_dev(self.h, self._st(stream), len(oo), elem, _addr(d_planes), _p64(po), _p64(ic),
                                                 d_n.data_ptr(), _addr(d_out), _p64(oo)), "hipd_merge_planes_dev")

    def split_planes_diff_dev(self, stream, elem, d_in, in_off, cap, d_n, d_planes, plane_off):
        """split_planes_dev of every element's difference to the element in front, zigzag-folded: with x[i] block b's elements as
        unsigned integers, x[-1] = 0 (every block starts afresh), plane j is byte j of z[i], the fold of (x[i] - x[i-1]) mod
        2^(8 elem).  split_planes_dev's arguments, and exactly its bytes written.  Enqueues only, one launch
        (include/shafa_hip.h: "Byte planes of differences")."""
        io, ic, po = _u64arr(in_off), _u64arr(cap), _u64arr(plane_off)
        _check(lib().shafa_hipd_split_planes_diff_dev(self.h, self._st(stream), len(io), elem, _addr(d_in), _p64(io), _p64(ic),
                                                      d_n.data_ptr(), _addr(d_planes), _p64(po)), "hipd_split_planes_diff_dev")

    def merge_planes_diff_dev(self, stream, elem, d_planes, plane_off, cap, d_n, d_out, out_off):
        """split_planes_diff_dev's inverse: the prefix sums (mod 2^(8 elem)) of the differences unfolded from block b's planes
        -> d_out + out_off[b].  merge_planes_dev's arguments, and exactly its bytes written.  Enqueues only: three launches, in
        none of which a workgroup waits for another (include/shafa_hip.h: "Byte planes of differences")."""
        oo, ic, po = _u64arr(out_off), _u64arr(cap), _u64arr(plane_off)
        _check(lib().shafa_hipd_merge_planes_diff_dev(self.h, self._st(stream), len(oo), elem, _addr(d_planes), _p64(po), _p64(ic),
                                                      d_n.data_ptr(), _addr(d_out), _p64(oo)), "hipd_merge_planes_diff_dev")

    def split_planes_lag_dev(self, stream, elem, lag, d_in, in_off, cap, d_n, d_planes, plane_off):
        """split_planes_dev of every element's difference to the element lag[b] >= 1 in front of it in block b (one lag a block;
        none in front: the element itself), zigzag-folded; lag 1 is split_planes_diff_dev byte for byte.  split_planes_dev's
        arguments, and exactly its bytes written, but the element side lies at multiples of elem: d_in and every in_off[b].
        Enqueues only, one launch (include/shafa_hip.h: "Byte planes of lagged differences")."""
        io, ic, po, lg = _u64arr(in_off), _u64arr(cap), _u64arr(plane_off), _u64arr(lag)
        if len(lg) != len(io):
            raise ValueError("split_planes_lag_dev: one lag per block")
        _check(lib().shafa_hipd_split_planes_lag_dev(self.h, self._st(stream), len(io), elem, _p64(lg), _addr(d_in), _p64(io),
                                                     _p64(ic), d_n.data_ptr(), _addr(d_planes), _p64(po)), "hipd_split_planes_lag_dev")

    def merge_planes_lag_dev(self, stream, elem, lag, d_planes, plane_off, cap, d_n, d_out, out_off):
        """split_planes_lag_dev's inverse: the prefix sums (mod 2^(8 elem)) down the lag[b] columns of the differences unfolded
        from block b's planes -> d_out + out_off[b], multiples of elem.  merge_planes_dev's arguments otherwise, and exactly its
        bytes written.  Enqueues only: up to three launches, in none of which a workgroup waits for another
        (include/shafa_hip.h: "Byte planes of lagged differences")."""
        oo, ic, po, lg = _u64arr(out_off), _u64arr(cap), _u64arr(plane_off), _u64arr(lag)
        if len(lg) != len(oo):
            raise ValueError("merge_planes_lag_dev: one lag per block")
        _check(lib().shafa_hipd_merge_planes_lag_dev(self.h, self._st(stream), len(oo), elem, _p64(lg), _addr(d_planes), _p64(po),
                                                     _p64(ic), d_n.data_ptr(), _addr(d_out), _p64(oo)), "hipd_merge_planes_lag_dev")

    def split_planes_grid_dev(self, stream, elem, lags, d_in, in_off, cap, d_n, d_planes, plane_off):
        """split_planes_lag_dev with up to PLANES_GRID_LAGS lags a block: `lags` is a list with one tuple per block, the first
        lag >= 1 and the others increasing (a trailing 0 is an unused slot; shorter tuples are padded with 0 to the call's
        widest), and the planes are those of the zigzag fold of d = (1 - S^L1)(1 - S^L2)(1 - S^L3) x mod 2^(8 elem): the
        differences along every lag in turn.  One lag a block is split_planes_lag_dev byte for byte.  Its arguments otherwise,
        and exactly its bytes written.  Enqueues only, one launch (include/shafa_hip.h: "Byte planes of Lorenzo differences")."""
        io, ic, po = _u64arr(in_off), _u64arr(cap), _u64arr(plane_off)
        nl, lg = _grid_lags("split_planes_grid_dev", lags, len(io))
        _check(lib().shafa_hipd_split_planes_grid_dev(self.h, self._st(stream), len(io), elem, nl, _p64(lg), _addr(d_in), _p64(io),
                                                      _p64(ic), d_n.data_ptr(), _addr(d_planes), _p64(po)),
               "hipd_split_planes_grid_dev")

    def merge_planes_grid_dev(self, stream, elem, lags, d_planes, plane_off, cap, d_n, d_out, out_off):
        """split_planes_grid_dev's inverse: the differences unfolded from block b's planes, then x[i] += x[i - L] once per lag of
        the block -> d_out + out_off[b], multiples of elem.  merge_planes_lag_dev's arguments otherwise, and exactly its bytes
        written.  Enqueues only: the first pass is the difference merge's launches (a smallest lag of 1) or the lag merge's, each
        further lag a pass in place over the elements; no workgroup waits for another (include/shafa_hip.h: "Byte planes of
        Lorenzo differences")."""
        oo, ic, po = _u64arr(out_off), _u64arr(cap), _u64arr(plane_off)
        nl, lg = _grid_lags("merge_planes_grid_dev", lags, len(oo))
        _check(lib().shafa_hipd_merge_planes_grid_dev(self.h, self._st(stream), len(oo), elem, nl, _p64(lg), _addr(d_planes),
                                                      _p64(po), _p64(ic), d_n.data_ptr(), _addr(d_out), _p64(oo)),
               "hipd_merge_planes_grid_dev")

    def split_planes_grid_quant_dev(self, stream, elem, lags, step, bound, d_in, in_off, cap, d_n, d_planes, plane_off, d_outl,
                                    outl_off, outl_cap, d_outl_n):
        """split_planes_grid_dev over the CODES of float (elem 4) or double (elem 8) elements under an error bound: `step` and
        `bound` are host floats, one per block, exactly representable in the element type; code = rint(x * T(1 / step)) as a
        signed integer, and the planes are split_planes_grid_dev's over the codes, byte for byte.  An element whose restored
        value T(code) * step misses `bound` — a NaN, an infinity and a value past the code range among them — is an outlier: its
        {position, bits} is written as two int64 at d_outl[2 * (outl_off[b] + slot)] while slot < outl_cap[b], and d_outl_n[b]
        (int64, zeroed by the call) counts the outliers FOUND, above the capacity too.  d_outl may be None where every capacity
        is 0.  Enqueues only: a memset and one launch (include/shafa_hip.h: "Error-bounded fields")."""
        io, ic, po, oo, oc = _u64arr(in_off), _u64arr(cap), _u64arr(plane_off), _u64arr(outl_off), _u64arr(outl_cap)
        nl, lg = _grid_lags("split_planes_grid_quant_dev", lags, len(io))
        sp, bd = _f64arr(step), _f64arr(bound)
        if not len(sp) == len(bd) == len(oo) == len(oc) == len(io):
            raise ValueError("split_planes_grid_quant_dev: one step, bound, record offset and record capacity per block")
        _check(lib().shafa_hipd_split_planes_grid_quant_dev(self.h, self._st(stream), len(io), elem, nl, _p64(lg), _pf64(sp), _pf64(bd),
                                                            _addr(d_in), _p64(io), _p64(ic), d_n.data_ptr(), _addr(d_planes),
                                                            _p64(po), None if d_outl is None else _addr(d_outl), _p64(oo), _p64(oc),
                                                            d_outl_n.data_ptr()), "hipd_split_planes_grid_quant_dev")

    def merge_planes_grid_quant_dev(self, stream, elem, lags, step, d_planes, plane_off, cap, d_n, d_outl, outl_off, outl_n, d_out,
                                    out_off):
        """split_planes_grid_quant_dev's inverse: merge_planes_grid_dev's chain gives the codes, a restore pass in place makes
        T(code) * step of each, and a patch pass stores the bits of block b's outl_n[b] (host) records from d_outl[2 *
        outl_off[b]] on at their positions.  A record whose position is at or past d_n[b] gives the block OUTSIDE_MODULE and is
        not written.  d_outl may be None where no block has a record.  Enqueues only (include/shafa_hip.h: "Error-bounded
        fields")."""
        oo, ic, po, ro, rn = _u64arr(out_off), _u64arr(cap), _u64arr(plane_off), _u64arr(outl_off), _u64arr(outl_n)
        nl, lg = _grid_lags("merge_planes_grid_quant_dev", lags, len(oo))
        sp = _f64arr(step)
        if not len(sp) == len(ro) == len(rn) == len(oo):
            raise ValueError("merge_planes_grid_quant_dev: one step, record offset and record count per block")
        _check(lib().shafa_hipd_merge_planes_grid_quant_dev(self.h, self._st(stream), len(oo), elem, nl, _p64(lg), _pf64(sp),
                                                            _addr(d_planes), _p64(po), _p64(ic), d_n.data_ptr(),
                                                            None if d_outl is None else _addr(d_outl), _p64(ro), _p64(rn),
                                                            _addr(d_out), _p64(oo)), "hipd_merge_planes_grid_quant_dev")

    def hist_planes_grid_dev(self, stream, elem, lags, d_in, in_off, cap, d_n, d_freq):
        """The histograms of the planes split_planes_grid_dev would write, without the planes: d_freq[(b * elem + j) * 256 + s]
        (int64) = how many of block b's d_n[b] elements have byte j of z equal to s.  `lags` as split_planes_grid_dev takes them,
        and () — a row of zeros — for plain planes: no difference, no fold, split_planes_dev's counts.  The blocks are only read
        and may overlap or coincide: one tensor, one block per candidate.  The element side at multiples of elem.  d_freq is
        hist256's layout with len(in_off) * elem histograms and is zeroed by the call; sf_build_codes and sf_encoded_size_dev
        take it as it is.  Enqueues only, one launch (include/shafa_hip.h: "Plane histograms of Lorenzo differences")."""
        io, ic = _u64arr(in_off), _u64arr(cap)
        nl, lg = _grid_lags("hist_planes_grid_dev", lags, len(io))
        _check(lib().shafa_hipd_hist_planes_grid_dev(self.h, self._st(stream), len(io), elem, nl, _p64(lg), _addr(d_in), _p64(io),
                                                     _p64(ic), d_n.data_ptr(), d_freq.data_ptr()), "hipd_hist_planes_grid_dev")

    def hist_planes_grid_quant_dev(self, stream, elem, lags, step, bound, d_in, in_off, cap, d_n, d_freq, d_outl_n):
        """hist_planes_grid_dev over the CODES of float (elem 4) or double (elem 8) elements under an error bound: d_freq (int64,
        its layout) counts the planes split_planes_grid_quant_dev would write for the same `lags`, `step` and `bound`, and
        d_outl_n[b] (int64) the elements it would record as outliers; neither a plane nor a record is written.  There is no
        plain candidate: () is refused.  The blocks are only read and may coincide: one tensor, one block per (lags, step).
        Both outputs are zeroed by the call.  Enqueues only, one launch (include/shafa_hip.h: "Field sizes under an error
        bound")."""
        io, ic = _u64arr(in_off), _u64arr(cap)
        nl, lg = _grid_lags("hist_planes_grid_quant_dev", lags, len(io))
        sp, bd = _f64arr(step), _f64arr(bound)
        if not len(sp) == len(bd) == len(io):
            raise ValueError("hist_planes_grid_quant_dev: one step and one bound per block")
        _check(lib().shafa_hipd_hist_planes_grid_quant_dev(self.h, self._st(stream), len(io), elem, nl, _p64(lg), _pf64(sp), _pf64(bd),
                                                           _addr(d_in), _p64(io), _p64(ic), d_n.data_ptr(), d_freq.data_ptr(),
                                                           d_outl_n.data_ptr()), "hipd_hist_planes_grid_quant_dev")

    def split_planes_grid_round_dev(self, stream, elem, lags, mant, keep, d_in, in_off, cap, d_n, d_planes, plane_off, d_outl,
                                    outl_off, outl_cap, d_outl_n):
        """split_planes_grid_quant_dev with another quantiser: the mantissa of every element rounded to keep[b] of its mant[b]
        bits, half to even, in integer arithmetic on the element's bits — elem 2 (mant 7: bfloat16, 10: float16; one call may mix
        them), 4 (23) or 8 (52), 0 <= keep <= mant, host ints, one per block.  The planes are split_planes_grid_dev's over the
        codes; a normal value that rounds up to Inf, a denormal or a NaN with a dropped bit set is an outlier, recorded as
        split_planes_grid_quant_dev records its own.  Enqueues only: a memset and one launch (include/shafa_hip.h: "Point-wise
        relative bounds")."""
        io, ic, po, oo, oc = _u64arr(in_off), _u64arr(cap), _u64arr(plane_off), _u64arr(outl_off), _u64arr(outl_cap)
        nl, lg = _grid_lags("split_planes_grid_round_dev", lags, len(io))
        mt, kp = _u32arr(mant), _u32arr(keep)
        if not len(mt) == len(kp) == len(oo) == len(oc) == len(io):
            raise ValueError("split_planes_grid_round_dev: one mant, keep, record offset and record capacity per block")
        _check(lib().shafa_hipd_split_planes_grid_round_dev(self.h, self._st(stream), len(io), elem, nl, _p64(lg), _pu32(mt), _pu32(kp),
                                                            _addr(d_in), _p64(io), _p64(ic), d_n.data_ptr(), _addr(d_planes),
                                                            _p64(po), None if d_outl is None else _addr(d_outl), _p64(oo), _p64(oc),
                                                            d_outl_n.data_ptr()), "hipd_split_planes_grid_round_dev")

    def merge_planes_grid_round_dev(self, stream, elem, lags, mant, keep, d_planes, plane_off, cap, d_n, d_outl, outl_off, outl_n,
                                    d_out, out_off):
        """split_planes_grid_round_dev's inverse: merge_planes_grid_dev's chain gives the codes, a restore pass in place makes the
        rounded bits of each (sign, |code| << (mant - keep)), and merge_planes_grid_quant_dev's patch pass stores the records' bits
        on top.  Its arguments with `mant` and `keep` for `step`.  Enqueues only (include/shafa_hip.h: "Point-wise relative
        bounds")."""
        oo, ic, po, ro, rn = _u64arr(out_off), _u64arr(cap), _u64arr(plane_off), _u64arr(outl_off), _u64arr(outl_n)
        nl, lg = _grid_lags("merge_planes_grid_round_dev", lags, len(oo))
        mt, kp = _u32arr(mant), _u32arr(keep)
        if not len(mt) == len(kp) == len(ro) == len(rn) == len(oo):
            raise ValueError("merge_planes_grid_round_dev: one mant, keep, record offset and record count per block")
        _check(lib().shafa_hipd_merge_planes_grid_round_dev(self.h, self._st(stream), len(oo), elem, nl, _p64(lg), _pu32(mt), _pu32(kp),
                                                            _addr(d_planes), _p64(po), _p64(ic), d_n.data_ptr(),
                                                            None if d_outl is None else _addr(d_outl), _p64(ro), _p64(rn),
                                                            _addr(d_out), _p64(oo)), "hipd_merge_planes_grid_round_dev")

    def hist_planes_grid_round_dev(self, stream, elem, lags, mant, keep, d_in, in_off, cap, d_n, d_freq, d_outl_n):
        """hist_planes_grid_quant_dev over split_planes_grid_round_dev's codes: d_freq counts the planes that split would write
        for the same `lags`, `mant` and `keep`, d_outl_n[b] the elements it would record; neither a plane nor a record is
        written.  The blocks are only read and may coincide: one tensor, one block per (lags, keep).  Both outputs are zeroed by
        the call.  Enqueues only, one launch (include/shafa_hip.h: "Point-wise relative bounds")."""
        io, ic = _u64arr(in_off), _u64arr(cap)
        nl, lg = _grid_lags("hist_planes_grid_round_dev", lags, len(io))
        mt, kp = _u32arr(mant), _u32arr(keep)
        if not len(mt) == len(kp) == len(io):
            raise ValueError("hist_planes_grid_round_dev: one mant and one keep per block")
        _check(lib().shafa_hipd_hist_planes_grid_round_dev(self.h, self._st(stream), len(io), elem, nl, _p64(lg), _pu32(mt), _pu32(kp),
                                                           _addr(d_in), _p64(io), _p64(ic), d_n.data_ptr(), d_freq.data_ptr(),
                                                           d_outl_n.data_ptr()), "hipd_hist_planes_grid_round_dev")

    def error_dev(self, stream, elem, mant, abs_bound, rel_bound, d_a, a_off, cap, d_n, d_ref, ref_off, d_stat):
        """The error statistics of what came back against the original: block b's d_n[b] <= cap[b] elements of `elem` = 2, 4 or 8
        bytes at d_a + a_off[b] (a decoder's or a merge's output: multiples of 16) against the elements at d_ref + ref_off[b]
        (any multiple of elem, read where they lie) -> the record of ERR_WORDS int64 at d_stat[12 b:]: counts, the two sums of
        squares, the largest error and its position, the originals' extremes, and how many finite elements err by more than
        abs_bound[b] + rel_bound[b] |x| (host floats, one per block; abs_bound may be inf).  mant[b]: the format's mantissa width
        (7: bfloat16, 10: float16).  Enqueues only, two launches (include/shafa_hip.h: "Error statistics")."""
        ao, ic, ro = _u64arr(a_off), _u64arr(cap), _u64arr(ref_off)
        mt, ab, rl = _u32arr(mant), _f64arr(abs_bound), _f64arr(rel_bound)
        if not len(mt) == len(ab) == len(rl) == len(ro) == len(ic) == len(ao):
            raise ValueError("error_dev: one mant, abs_bound, rel_bound, offset and capacity per block")
        _check(lib().shafa_hipd_error_dev(self.h, self._st(stream), len(ao), elem, _pu32(mt), _pf64(ab), _pf64(rl), _addr(d_a), _p64(ao),
                                          _p64(ic), d_n.data_ptr(), _addr(d_ref), _p64(ro), d_stat.data_ptr()), "hipd_error_dev")

    def error_quant_dev(self, stream, elem, step, bound, d_in, in_off, cap, d_n, d_stat):
        """error_dev's record of the blocks at d_in + in_off[b] (elem 4 or 8) against what merge_planes_grid_quant_dev would give
        back for step[b] and bound[b], made in registers: no planes, no records, no second tensor; word 4 counts the outliers,
        which come back bit for bit.  The blocks are only read and may coincide: one tensor, one block per bound.  Enqueues
        only, two launches (include/shafa_hip.h: "Error statistics")."""
        io, ic = _u64arr(in_off), _u64arr(cap)
        sp, bd = _f64arr(step), _f64arr(bound)
        if not len(sp) == len(bd) == len(ic) == len(io):
            raise ValueError("error_quant_dev: one step, bound, offset and capacity per block")
        _check(lib().shafa_hipd_error_quant_dev(self.h, self._st(stream), len(io), elem, _pf64(sp), _pf64(bd), _addr(d_in), _p64(io),
                                                _p64(ic), d_n.data_ptr(), d_stat.data_ptr()), "hipd_error_quant_dev")

    def error_round_dev(self, stream, elem, mant, keep, d_in, in_off, cap, d_n, d_stat):
        """error_quant_dev under the rounding rule: elem 2, 4 or 8, keep[b] of the format's mant[b] mantissa bits kept, as
        hist_planes_grid_round_dev takes them.  Enqueues only, two launches (include/shafa_hip.h: "Error statistics")."""
        io, ic = _u64arr(in_off), _u64arr(cap)
        mt, kp = _u32arr(mant), _u32arr(keep)
        if not len(mt) == len(kp) == len(ic) == len(io):
            raise ValueError("error_round_dev: one mant, keep, offset and capacity per block")
        _check(lib().shafa_hipd_error_round_dev(self.h, self._st(stream), len(io), elem, _pu32(mt), _pu32(kp), _addr(d_in), _p64(io),
                                                _p64(ic), d_n.data_ptr(), d_stat.data_ptr()), "hipd_error_round_dev")

    def split_planes_xor_dev(self, stream, elem, d_in, in_off, d_base, base_off, cap, d_n, d_planes, plane_off):
        """split_planes_dev of (element XOR base element): block b's base is its elem * d_n[b] bytes at d_base + base_off[b],
        at any alignment of its own, read in place and once; base_off[b] == PLANES_NO_BASE: the block has none and comes out as
        split_planes_dev's, nothing is read through d_base for it.  The bases must not overlap the planes.  d_base is a tensor
        or a device address (int).  Enqueues only (include/shafa_hip.h: "Byte planes of deltas")."""
        io, bo, ic, po = _u64arr(in_off), _u64arr(base_off), _u64arr(cap), _u64arr(plane_off)
        if len(bo) != len(io):
            raise ValueError("split_planes_xor_dev: one base offset per block")
        _check(lib().shafa_hipd_split_planes_xor_dev(self.h, self._st(stream), len(io), elem, _addr(d_in), _p64(io), _addr(d_base),
                                                     _p64(bo), _p64(ic), d_n.data_ptr(), _addr(d_planes), _p64(po)),
               "hipd_split_planes_xor_dev")

    def merge_planes_xor_dev(self, stream, elem, d_planes, plane_off, d_base, base_off, cap, d_n, d_out, out_off):
        """split_planes_xor_dev's inverse: (the elements put together from block b's planes) XOR its base at d_base +
        base_off[b] (any alignment; PLANES_NO_BASE: none, merge_planes_dev's result) -> d_out + out_off[b]; no other byte of
        d_out is written.  The bases must not overlap the output regions: merging in place is not supported.  Enqueues only
        (include/shafa_hip.h: "Byte planes of deltas")."""
        po, bo, ic, oo = _u64arr(plane_off), _u64arr(base_off), _u64arr(cap), _u64arr(out_off)
        if len(bo) != len(oo):
            raise ValueError("merge_planes_xor_dev: one base offset per block")
        _check(lib().shafa_hipd_merge_planes_xor_dev(self.h, self._st(stream), len(oo), elem, _addr(d_planes), _p64(po),
                                                     _addr(d_base), _p64(bo), _p64(ic), d_n.data_ptr(), _addr(d_out), _p64(oo)),
               "hipd_merge_planes_xor_dev")

    def split_records_dev(self, stream, width, d_in, in_off, cap, d_n, d_planes, plane_off):
        """Block b's d_n[b] (int64, device; <= cap[b]) RECORDS of `width` = 1 .. RECORDS_MAX_WIDTH bytes at d_in + in_off[b]
        (bytes, any alignment, read in place) -> their byte columns: column j (byte j of every record) is d_n[b] bytes at
        d_planes + plane_off[b * width + j].  d_planes and every column offset are multiples of 16; nothing behind a column's
        d_n[b] bytes is written.  At width 1, 2, 4, 8 the bytes are split_planes_dev's.  d_in and d_planes are tensors or device
        addresses (int).  Enqueues only (include/shafa_hip.h: "Byte columns of fixed-width records")."""
        io, ic, po = _u64arr(in_off), _u64arr(cap), _u64arr(plane_off)
        _check(lib().shafa_hipd_split_records_dev(self.h, self._st(stream), len(io), width, _addr(d_in), _p64(io), _p64(ic),
                                                  d_n.data_ptr(), _addr(d_planes), _p64(po)), "hipd_split_records_dev")

    def merge_records_dev(self, stream, width, d_planes, plane_off, cap, d_n, d_out, out_off):
        """split_records_dev's inverse: block b's columns (d_n[b] bytes each at d_planes + plane_off[b * width + j], multiples
        of 16) -> its width * d_n[b] bytes at d_out + out_off[b] (any alignment); no other byte of d_out is written, the up to
        15 bytes on either side of an unaligned region included.  d_planes and d_out are tensors or device addresses (int).
        Enqueues only (include/shafa_hip.h: "Byte columns of fixed-width records")."""
        po, ic, oo = _u64arr(plane_off), _u64arr(cap), _u64arr(out_off)
        _check(lib().shafa_hipd_merge_records_dev(self.h, self._st(stream), len(oo), width, _addr(d_planes), _p64(po), _p64(ic),
                                                  d_n.data_ptr(), _addr(d_out), _p64(oo)), "hipd_merge_records_dev")

    def seek_index_dev(self, stream, d_in, in_off, in_cap, d_in_n, d_tables, span, flags, ckpt_first, d_ckpt, d_status, d_out_n):
        """The checkpoints, every `span` symbols, of blocks of SF-decoded bytes: block b's d_in_n[b] (int64, device; <=
        in_cap[b]) bytes at d_in + in_off[b], with d_tables[b] (device; None without SEEK_SF) -> d_ckpt (int64, two words a
        checkpoint, block b's from checkpoint ckpt_first[b]), d_status[b] (int32) and d_out_n[b] (int64, the decoded size).
        Enqueues only (include/shafa_hip.h: "Seek index")."""
        io, ic, cf = _u64arr(in_off), _u64arr(in_cap), _u64arr(ckpt_first)
        _check(lib().shafa_hipd_seek_index_dev(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(ic),
                                               d_in_n.data_ptr(), None if d_tables is None else d_tables.data_ptr(), span,
                                               flags, _p64(cf), d_ckpt.data_ptr(), d_status.data_ptr(), d_out_n.data_ptr()),
               "hipd_seek_index_dev")

    def read_spans_dev(self, stream, d_file, pay_off, pay_n, n_symbols, ckpt_first, d_tables, span, flags, d_ckpt, items, d_out):
        """The ranged decoder: items = (block, first checkpoint, last checkpoint, lo, hi, destination offset), the blocks
        described by the four host sequences; item i's code is word i of finish.  Enqueues only (include/shafa_hip.h:
        shafa_hipd_read_spans_dev)."""
        po, pn, ns, cf = _u64arr(pay_off), _u64arr(pay_n), _u64arr(n_symbols), _u64arr(ckpt_first)
        it = np.asarray(items, dtype=np.uint64).reshape(-1, 6)
        blk = _i32arr(it[:, 0])
        col = [_u64arr(it[:, k]) for k in range(1, 6)]
        _check(lib().shafa_hipd_read_spans_dev(self.h, self._st(stream), len(po), _ptr(d_file), d_file.numel(), _p64(po), _p64(pn),
                                               _p64(ns), _p64(cf), None if d_tables is None else d_tables.data_ptr(), span, flags,
                                               d_ckpt.data_ptr(), len(blk), _p32(blk), *[_p64(c) for c in col], d_out.data_ptr(),
                                               d_out.numel()), "hipd_read_spans_dev")

    def sf_decode(self, stream, d_in, in_off, in_n, tables, n_symbols, d_out, out_off):
        io, il, oo, ns = _u64arr(in_off), _u64arr(in_n), _u64arr(out_off), _u64arr(n_symbols)
        tarr = tables if isinstance(tables, C.Array) else self._tables(tables)
        _check(lib().shafa_hipd_sf_decode(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(il),
                                          tarr, _p64(ns), d_out.data_ptr(), _p64(oo)), "hipd_sf_decode")

    def rle_decode(self, stream, d_in, in_off, in_n, d_out, out_off, out_cap, d_out_n):
        io, il, oo, oc = _u64arr(in_off), _u64arr(in_n), _u64arr(out_off), _u64arr(out_cap)
        _check(lib().shafa_hipd_rle_decode(self.h, self._st(stream), len(io), d_in.data_ptr(), _p64(io), _p64(il),
                                           d_out.data_ptr(), _p64(oo), _p64(oc), d_out_n.data_ptr()), "hipd_rle_decode")

    # ---- files in device memory (include/shafa_hip.h: "Files in device memory"); enqueue only, d_dst_n: 1 int64 ----
    def pack_payloads(self, stream, framing, d_src, src_off, src_cap, d_src_n, d_dst, dst_cap, d_dst_n):
        """block b's d_src_n[b] (<= src_cap[b]) bytes at d_src + src_off[b] -> one .rle (FRAME_RAW) or .shaf (FRAME_SHAF)
        file at d_dst; its length to d_dst_n[0]."""
        so, sc = _u64arr(src_off), _u64arr(src_cap)
        _check(lib().shafa_hipd_pack_payloads(self.h, self._st(stream), len(so), framing, d_src.data_ptr(), _p64(so),
                                              _p64(sc), d_src_n.data_ptr(), d_dst.data_ptr(), int(dst_cap),
                                              d_dst_n.data_ptr()), "hipd_pack_payloads")

    def pack_cod(self, stream, nblocks, mode, d_sizes, d_tables, d_dst, dst_cap, d_dst_n):
        """.cod file of nblocks device tables (d_tables: nblocks x sizeof(CodeTable) bytes) headed by d_sizes (int64)."""
        _check(lib().shafa_hipd_pack_cod(self.h, self._st(stream), nblocks, _mode(mode), d_sizes.data_ptr(),
                                         d_tables.data_ptr(), d_dst.data_ptr(), int(dst_cap), d_dst_n.data_ptr()),
               "hipd_pack_cod")

    def pack_freq(self, stream, nblocks, mode, d_sizes, d_freq, d_dst, dst_cap, d_dst_n):
        """.freq file of nblocks x 256 device counts (d_freq, int64) headed by d_sizes (int64)."""
        _check(lib().shafa_hipd_pack_freq(self.h, self._st(stream), nblocks, _mode(mode), d_sizes.data_ptr(),
                                          d_freq.data_ptr(), d_dst.data_ptr(), int(dst_cap), d_dst_n.data_ptr()),
               "hipd_pack_freq")

    # ---- many files per call (include/shafa_hip.h: "Many files per call"); enqueue only, d_dst_n: nfiles int64 ----
    # file f is blocks first[f] .. first[f] + count[f] - 1, written at d_dst + dst_off[f] in dst_cap[f] bytes
    def pack_payloads_files(self, stream, first, count, framing, d_src, src_off, src_cap, d_src_n, d_dst, dst_off, dst_cap,
                            d_dst_n):
        """pack_payloads per file: .rle (FRAME_RAW) or .shaf (FRAME_SHAF) files of the blocks' d_src_n[b] bytes at
        d_src + src_off[b]."""
        fi, co, so, sc, do, dc = _i32arr(first), _i32arr(count), _u64arr(src_off), _u64arr(src_cap), _u64arr(dst_off), \
            _u64arr(dst_cap)
        _check(lib().shafa_hipd_pack_payloads_files(self.h, self._st(stream), len(fi), _p32(fi), _p32(co), framing,
                                                    d_src.data_ptr(), _p64(so), _p64(sc), d_src_n.data_ptr(),
                                                    d_dst.data_ptr(), _p64(do), _p64(dc), d_dst_n.data_ptr()),
               "hipd_pack_payloads_files")

    def pack_cod_files(self, stream, first, count, modes, d_sizes, d_tables, d_dst, dst_off, dst_cap, d_dst_n):
        """pack_cod per file, file f in mode modes[f] (b"R" / b"N")."""
        fi, co, do, dc = _i32arr(first), _i32arr(count), _u64arr(dst_off), _u64arr(dst_cap)
        _check(lib().shafa_hipd_pack_cod_files(self.h, self._st(stream), len(fi), _p32(fi), _p32(co), _modes(modes),
                                               d_sizes.data_ptr(), d_tables.data_ptr(), d_dst.data_ptr(), _p64(do),
                                               _p64(dc), d_dst_n.data_ptr()), "hipd_pack_cod_files")

    def pack_freq_files(self, stream, first, count, modes, d_sizes, d_freq, d_dst, dst_off, dst_cap, d_dst_n):
        """pack_freq per file, file f in mode modes[f] (b"R" / b"N")."""
        fi, co, do, dc = _i32arr(first), _i32arr(count), _u64arr(dst_off), _u64arr(dst_cap)
        _check(lib().shafa_hipd_pack_freq_files(self.h, self._st(stream), len(fi), _p32(fi), _p32(co), _modes(modes),
                                                d_sizes.data_ptr(), d_freq.data_ptr(), d_dst.data_ptr(), _p64(do),
                                                _p64(dc), d_dst_n.data_ptr()), "hipd_pack_freq_files")

    # ---- files in device memory, parsed (include/shafa_hip.h: "Files in device memory, parsed"); enqueue only ----
    # d_info: UNPACK_INFO_WORDS int64; d_sizes / d_off / d_n: max_blocks int64; d_tables: max_blocks x sizeof(CodeTable) bytes
    def unpack_cod(self, stream, max_blocks, d_cod, d_info, d_sizes, d_tables):
        """.cod file (uint8 tensor, any alignment) -> header info, symbol counts and code tables of its first max_blocks blocks."""
        _check(lib().shafa_hipd_unpack_cod(self.h, self._st(stream), max_blocks, _ptr(d_cod), d_cod.numel(), d_info.data_ptr(),
                                           d_sizes.data_ptr(), d_tables.data_ptr()), "hipd_unpack_cod")

    def unpack_rle_freq(self, stream, max_blocks, d_freq, rle_n, d_info, d_off, d_n):
        """.rle.freq file -> header info and block b's payload [d_off[b], d_off[b] + d_n[b]) in a .rle file of rle_n bytes."""
        _check(lib().shafa_hipd_unpack_rle_freq(self.h, self._st(stream), max_blocks, _ptr(d_freq), d_freq.numel(), int(rle_n),
                                                d_info.data_ptr(), d_off.data_ptr(), d_n.data_ptr()), "hipd_unpack_rle_freq")

    def unpack_freq(self, stream, max_blocks, d_freq_text, d_info, d_sizes, d_counts):
        """.freq / .rle.freq file, its counts parsed -> header info, block sizes and d_counts (max_blocks x 256 int64: what
        sf_build_codes and pack_freq take)."""
        _check(lib().shafa_hipd_unpack_freq(self.h, self._st(stream), max_blocks, _ptr(d_freq_text), d_freq_text.numel(),
                                            d_info.data_ptr(), d_sizes.data_ptr(), d_counts.data_ptr()), "hipd_unpack_freq")

    def unpack_shaf(self, stream, max_blocks, d_shaf, d_count, d_off, d_n):
        """.shaf file -> block b's payload [d_off[b], d_off[b] + d_n[b]) for min(d_count[0], max_blocks) blocks."""
        _check(lib().shafa_hipd_unpack_shaf(self.h, self._st(stream), max_blocks, _ptr(d_shaf), d_shaf.numel(),
                                            d_count.data_ptr(), d_off.data_ptr(), d_n.data_ptr()), "hipd_unpack_shaf")

    def unpack_payloads(self, stream, d_file, d_off, d_n, d_dst, dst_off, dst_cap):
        """block b's payload (d_off / d_n: device int64) -> d_dst + dst_off[b] (16-aligned regions of dst_cap[b] bytes)."""
        do, dc = _u64arr(dst_off), _u64arr(dst_cap)
        _check(lib().shafa_hipd_unpack_payloads(self.h, self._st(stream), len(do), _ptr(d_file), d_file.numel(),
                                                d_off.data_ptr(), d_n.data_ptr(), d_dst.data_ptr(), _p64(do), _p64(dc)),
               "hipd_unpack_payloads")

    def unpack_payloads_at(self, stream, file_addr, file_n, d_off, d_n, d_dst, dst_off, dst_cap):
        """unpack_payloads from the file [file_addr, file_addr + file_n) given by its device address (int): the base the
        segmented parses measure offsets from, which spans many tensors."""
        do, dc = _u64arr(dst_off), _u64arr(dst_cap)
        _check(lib().shafa_hipd_unpack_payloads(self.h, self._st(stream), len(do), file_addr or None, int(file_n),
                                                d_off.data_ptr(), d_n.data_ptr(), d_dst.data_ptr(), _p64(do), _p64(dc)),
               "hipd_unpack_payloads")

    # ---- many files per call, parsed (include/shafa_hip.h: "Many files per call, parsed"); enqueue only ----
    # file f: n[f] bytes at base + off[f] (base: a device address, int); its blocks take slots first[f] .. first[f] +
    # max_blocks[f] - 1 of the per-slot arrays; its record: d_info[f * UNPACK_INFO_WORDS:]
    def unpack_cod_files(self, stream, first, max_blocks, base, off, n, d_info, d_sizes, d_tables):
        """unpack_cod per file: header records, symbol counts and code tables per slot."""
        fi, mb, o, nn = _i32arr(first), _i32arr(max_blocks), _u64arr(off), _u64arr(n)
        _check(lib().shafa_hipd_unpack_cod_files(self.h, self._st(stream), len(fi), _p32(fi), _p32(mb), base or None, _p64(o),
                                                 _p64(nn), d_info.data_ptr(), d_sizes.data_ptr(), d_tables.data_ptr()),
               "hipd_unpack_cod_files")

    def unpack_rle_freq_files(self, stream, first, max_blocks, base, off, n, rle_off, rle_n, d_info, d_off, d_n):
        """unpack_rle_freq per file: file f's .rle is rle_n[f] bytes at rle_off[f] from the call's .rle base, which d_off
        is measured from."""
        fi, mb, o, nn, ro, rn = _i32arr(first), _i32arr(max_blocks), _u64arr(off), _u64arr(n), _u64arr(rle_off), \
            _u64arr(rle_n)
        _check(lib().shafa_hipd_unpack_rle_freq_files(self.h, self._st(stream), len(fi), _p32(fi), _p32(mb), base or None,
                                                      _p64(o), _p64(nn), _p64(ro), _p64(rn), d_info.data_ptr(),
                                                      d_off.data_ptr(), d_n.data_ptr()), "hipd_unpack_rle_freq_files")

    def unpack_shaf_files(self, stream, first, max_blocks, base, off, n, d_count, d_off, d_n):
        """unpack_shaf per file, its block count at d_count[f * UNPACK_INFO_WORDS] (d_info[INFO_INDEXED:] of
        unpack_cod_files); d_off is measured from base."""
        fi, mb, o, nn = _i32arr(first), _i32arr(max_blocks), _u64arr(off), _u64arr(n)
        _check(lib().shafa_hipd_unpack_shaf_files(self.h, self._st(stream), len(fi), _p32(fi), _p32(mb), base or None,
                                                  _p64(o), _p64(nn), d_count.data_ptr(), d_off.data_ptr(), d_n.data_ptr()),
               "hipd_unpack_shaf_files")

    def finish(self, stream, nblocks, raise_on_error=True):
        errs = (C.c_int * max(nblocks, 1))()
        rc = lib().shafa_hipd_finish(self.h, self._st(stream), nblocks, errs)
        if raise_on_error:
            _check(rc, "hipd_finish")
        return rc, list(errs)[:nblocks]


class Pipe:
    """Layer 3: bounded in-order block pipeline over host buffers (shafa_pipe_*)."""

    def __init__(self, n_slots):
        self._h = C.c_void_p()
        _check(lib().shafa_pipe_create(n_slots, C.byref(self._h)), "pipe_create")
        self.n_slots = lib().shafa_pipe_slots(self._h)
        self.devices = [lib().shafa_pipe_slot_device(self._h, i) for i in range(self.n_slots)]

    def close(self):
        if self._h:
            lib().shafa_pipe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, slot, op, data, table=None, n_symbols=0, out_cap=0, flags=0):
        a = _np_u8(data)
        p = lib().shafa_pipe_in(self._h, slot, a.size)
        if not p:
            raise ShafaError(LACK_OF_MEMORY, "pipe_in (slot busy?)")
        C.memmove(p, a.ctypes.data, a.size)
        _check(lib().shafa_pipe_submit(self._h, slot, op, a.size, C.byref(table) if table is not None else None,
                                       n_symbols, out_cap, flags), "pipe_submit")

    def wait(self, slot, raw_rc=False):
        """-> (rc, result bytes, PipeResult)"""
        r = PipeResult()
        rc = lib().shafa_pipe_wait(self._h, slot, C.byref(r))
        if rc and not raw_rc:
            _check(rc, "pipe_wait")
        out = C.string_at(r.out, r.out_n) if rc == 0 and r.out_n else b""
        return rc, out, r


    def ftc_encode(self, slot, use_rle, table, out_cap):
        """stage two of SHAFA_OP_FTC: Module C from the bytes stage one left on the device (shafa_pipe_ftc_encode)"""
        _check(lib().shafa_pipe_ftc_encode(self._h, slot, 1 if use_rle else 0, C.byref(table), out_cap), "pipe_ftc_encode")

    def submit_group(self, slot, op, datas, tables=None, n_symbols=None, out_caps=None, flags=0):
        """several blocks in one slot: inputs laid out at 16-byte aligned offsets (shafa_pipe_submit_group)"""
        arrs = [_np_u8(d) for d in datas]
        offs, pos = [], 0
        for a in arrs:
            offs.append(pos)
            pos += (a.size + 15) // 16 * 16
        p = lib().shafa_pipe_in(self._h, slot, max(pos, 16))
        if not p:
            raise ShafaError(LACK_OF_MEMORY, "pipe_in (slot busy?)")
        blocks = (PipeBlock * len(arrs))()
        self._keep = tables                                   # the tables must outlive the call
        for i, a in enumerate(arrs):
            if a.size:
                C.memmove(p + offs[i], a.ctypes.data, a.size)
            blocks[i].in_off, blocks[i].in_n = offs[i], a.size
            blocks[i].table = C.pointer(tables[i]) if tables is not None else None
            blocks[i].n_symbols = n_symbols[i] if n_symbols is not None else 0
            blocks[i].out_cap = out_caps[i] if out_caps is not None else 0
        _check(lib().shafa_pipe_submit_group(self._h, slot, op, len(arrs), blocks, flags), "pipe_submit_group")
        return len(arrs)

    def wait_group(self, slot, n):
        """-> (rc of the call, [block rc], [result bytes], [PipeResult])"""
        res = (PipeResult * n)()
        brc = (C.c_int * n)()
        rc = lib().shafa_pipe_wait_group(self._h, slot, n, res, brc)
        outs = [C.string_at(res[i].out, res[i].out_n) if rc == 0 and brc[i] == 0 and res[i].out_n else b"" for i in range(n)]
        return rc, list(brc), outs, res


FRAME_RAW, FRAME_SHAF = 0, 1   # SHAFA_FRAME_*: .rle (payloads back to back), .shaf ("@n", then "@size@" + payload)


def _mode(mode):
    return C.c_char(mode if isinstance(mode, bytes) else str(mode).encode())


def _modes(modes):
    """per-file modes (b"RN..", or a sequence of b"R" / "N") as a C string"""
    if isinstance(modes, bytes):
        return modes
    return b"".join(m if isinstance(m, bytes) else str(m).encode() for m in modes)


def pack_payloads_max(src_cap, framing):
    """bytes that Batch.pack_payloads may need for blocks of these capacities (shafa_hip_pack_payloads_max)."""
    sc = _u64arr(src_cap)
    return int(lib().shafa_hip_pack_payloads_max(len(sc), _p64(sc), framing))


def pack_cod_max(nblocks):
    return int(lib().shafa_hip_pack_cod_max(nblocks))


def pack_freq_max(nblocks):
    return int(lib().shafa_hip_pack_freq_max(nblocks))


TILE_BYTES = 32768            # SHAFA_TILE_BYTES: the tile of the tile histograms


def tile_hist_bytes(n):
    """bytes of the tile histograms of a block of n bytes (256 x u16 per 32 KiB tile)."""
    return int(lib().shafa_hip_tile_hist_bytes(int(n)))


def gen_bytes(stream, seed, first_index, d_out, n, d_map=None):
    st = C.c_void_p(stream.cuda_stream) if stream is not None else None
    _check(lib().shafa_hipd_gen_bytes(st, seed, first_index, d_map.data_ptr() if d_map is not None else None,
                                      d_out.data_ptr(), n), "hipd_gen_bytes")


def zipf_table(s=1.2, nsym=256):
    """2^16-entry inverse CDF of Zipf(s) over nsym symbols: the byte map of the synthetic streams
    (SURVEY.md §8(d) config 4).  Same construction as tests/golden/make_golden.py."""
    w = np.arange(1, nsym + 1, dtype=np.float64) ** (-s)
    cdf = np.cumsum(w) / np.sum(w)
    edges = np.minimum(np.floor(cdf * 65536.0 + 0.5).astype(np.int64), 65536)
    edges[-1] = 65536
    table = np.zeros(65536, dtype=np.uint8)
    lo = 0
    for k in range(nsym):
        table[lo:edges[k]] = k
        lo = max(lo, edges[k])
    return table


# ------------------------------------------------------------------ C host library (formats, Module T, drivers)
_host = None


def host():
    """Load libshafa_host.so: the C host's formats, Module T and module drivers (host/shafa_host.h)."""
    global _host
    if _host is not None:
        return _host
    lib()   # libshafa_host.so links against libshafa_hip.so
    path = os.environ.get("SHAFA_HOST_LIB") or HOST_LIB_PATH        # (the sanitizer build of tools/san/run_san.sh)
    if not os.path.exists(path):
        raise ImportError(f"{path} not built: run __graft_entry__.build()")
    H = C.CDLL(path)
    u64p, tp = C.POINTER(C.c_uint64), C.POINTER(CodeTable)
    H.shafa_sf_build_codes.argtypes = [u64p, tp]
    H.shafa_sf_build_codes.restype = None
    H.shafa_sf_build_codes_batch.argtypes = [u64p, C.c_int, tp]
    H.shafa_sf_build_codes_batch.restype = None
    H.shafa_freq_format.argtypes = [u64p, C.c_char_p]
    H.shafa_freq_format.restype = C.c_size_t
    H.shafa_freq_parse.argtypes = [C.c_char_p, u64p]
    H.shafa_cod_format.argtypes = [tp, C.c_char_p]
    H.shafa_cod_format.restype = C.c_size_t
    H.shafa_cod_parse.argtypes = [C.c_char_p, tp]
    H.shafa_rle_worthwhile.argtypes = [C.c_uint64, C.c_uint64, C.c_bool]
    H.shafa_rle_worthwhile.restype = C.c_bool
    H.shafa_block_count.argtypes = [C.c_uint64, u64p, u64p]
    H.shafa_block_count.restype = C.c_uint64
    _host = H
    return H


def sf_build_codes(freq):
    """Module T core (reference t.c:74-210) on one 256-bin histogram -> CodeTable."""
    f = np.ascontiguousarray(freq, dtype=np.uint64)
    t = CodeTable()
    host().shafa_sf_build_codes(f.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(t))
    return t


def sf_build_codes_batch(freq):
    """Module T on n histograms (array n x 256) -> ctypes array of n CodeTable (what Batch.sf_encode / sf_decode take)."""
    f = np.ascontiguousarray(freq, dtype=np.uint64).reshape(-1, 256)
    arr = (CodeTable * f.shape[0])()
    host().shafa_sf_build_codes_batch(f.ctypes.data_as(C.POINTER(C.c_uint64)), f.shape[0], arr)
    return arr


def freq_format(freq):
    f = np.ascontiguousarray(freq, dtype=np.uint64)
    buf = C.create_string_buffer(256 * 21 + 1)
    n = host().shafa_freq_format(f.ctypes.data_as(C.POINTER(C.c_uint64)), buf)
    return buf.raw[:n]


def freq_parse(text):
    f = np.zeros(256, dtype=np.uint64)
    rc = host().shafa_freq_parse(text, f.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, f


def cod_format(table):
    buf = C.create_string_buffer(33152 + 8)
    n = host().shafa_cod_format(C.byref(table), buf)
    return buf.raw[:n]


def cod_parse(text):
    t = CodeTable()
    rc = host().shafa_cod_parse(text, C.byref(t))
    return rc, t


# ------------------------------------------------------------------ F -> T -> C into files, in device memory
def _al16(x):
    return (x + 15) // 16 * 16


def _stream(dev, stream):
    """the stream a driver works on: the caller's, or a new one on dev"""
    import torch
    return stream if stream is not None else torch.cuda.Stream(device=dev)


def _max_bytes(dev, max_bytes):
    """a driver's working-memory budget: the caller's, or a quarter of what is free on dev"""
    import torch
    return torch.cuda.mem_get_info(dev)[0] // 4 if max_bytes is None else max_bytes


def _aligned_blocks(bt, st, src, starts, sizes, d_sizes):
    """The blocks of `src` at `starts` with these sizes (d_sizes: the sizes on the device) at 16-byte aligned addresses, the
    device entries' rule: in place when they are, else gathered by one unpack_payloads -> (tensor, offsets)"""
    import torch
    if not src.data_ptr() % 16 and not any(o % 16 for o in starts):
        return src, list(starts)
    off, tot = _layout(sizes)
    buf = torch.empty(tot + 16, dtype=torch.uint8, device=src.device)
    bt.unpack_payloads(st, src, torch.tensor(starts, dtype=torch.int64, device=src.device), d_sizes, buf, off, sizes)
    return buf, off


def compress_files(d_in, block_size, force_rle=False, force_freq=False, stream=None):
    """The files the CLI's default run `shafa <file> -b <size> [-c r|f]` writes for the bytes of `d_in` (a contiguous uint8
    CUDA tensor, any alignment), made on the device: {".rle", ".rle.freq", ".freq", ".rle.cod", ".rle.shaf"} with RLE (".freq"
    only with force_freq), {".freq", ".cod", ".shaf"} without.  Each value is a uint8 CUDA tensor holding exactly the file.
    This is compress_many's chain on one file (one group, whatever its block count): see there.  Raises
    ShafaError(FILE_TOO_SMALL) below 1 KiB before any device work, else the file's first error in block order, an error of
    the size pass in front of a later stage's."""
    entry, = _per_group("compress_files", d_in, [int(d_in.numel())], block_size, stream,
                        lambda g: _compress_group(g, force_rle, force_freq))
    if isinstance(entry, ShafaError):
        raise entry
    return entry


MANY_GROUP_BLOCKS = 16384      # compress_many: blocks per device batch (the F / T / C launches put blocks on the grid's y)


def _many_files(name, d_in, sizes, block_size):
    """compress_many's arguments checked -> (d_in as one tensor, sizes, each file's start in d_in, {file: its block sizes} by
    the C host's split (shafa_block_count) for the files of 1 KiB or more, groups of those files): a group holds at most
    MANY_GROUP_BLOCKS blocks.  A file alone is one group whatever its block count."""
    import torch
    if isinstance(d_in, (list, tuple)):
        if sizes is None:
            sizes = [int(t.numel()) for t in d_in]
        d_in = torch.cat([t.reshape(-1) for t in d_in]) if d_in else None
    sizes = [int(n) for n in (sizes or [])]
    if not sizes:
        raise ValueError(f"{name}: no files")
    if d_in is None or not isinstance(d_in, torch.Tensor) or d_in.dtype != torch.uint8 or not d_in.is_cuda \
            or not d_in.is_contiguous():
        raise ValueError(f"{name}: d_in is a contiguous uint8 CUDA tensor")
    if sum(sizes) > d_in.numel() or min(sizes) < 0:
        raise ValueError(f"{name}: sizes exceed d_in")
    start, pos = [], 0
    for n in sizes:
        start.append(pos)
        pos += n
    split = {}
    for f, n in enumerate(sizes):
        if n >= 1024:
            bs, last = C.c_uint64(int(block_size)), C.c_uint64(0)
            nb = int(host().shafa_block_count(n, C.byref(bs), C.byref(last)))
            split[f] = [bs.value] * (nb - 1) + [last.value]
    groups, group, acc = [], [], 0
    for f in split:
        k = len(split[f])
        if group and acc + k > MANY_GROUP_BLOCKS:
            groups.append(group)
            group, acc = [], 0
        group.append(f)
        acc += k
    if group:
        groups.append(group)
    return d_in, sizes, start, split, groups


def _per_group(name, d_in, sizes, block_size, stream, body):
    """The compress drivers' prelude: the arguments checked, split and grouped (_many_files), then body(group) -> the
    entries of that group's files, for each group on its own batch -> one entry per file, for a file under 1 KiB a
    ShafaError(FILE_TOO_SMALL) instance, settled before any device work (f.c:220,366)."""
    d_in, sizes, start, split, groups = _many_files(name, d_in, sizes, block_size)
    results = [None if f in split else ShafaError(FILE_TOO_SMALL, f"{name}: fewer than 1024 bytes")
               for f in range(len(sizes))]
    st = _stream(d_in.device, stream) if groups else None
    for group in groups:
        with _GroupBlocks(name, d_in, start, split, group, st) as g:
            entries = body(g)
            for f, entry in zip(g.files, entries):                         # g.files: as the body left them (rle_first)
                results[f] = entry
    return results


def compress_many(d_in, sizes=None, block_size=65536, force_rle=False, force_freq=False, stream=None):
    """compress_files for many files in one device batch.  `d_in` holds the files back to back (a contiguous uint8 CUDA tensor;
    a list of such tensors is concatenated), `sizes` their lengths (for a list: None = the tensors' lengths).  Returns one entry
    per file: the dict compress_files returns for that file alone, byte for byte, or a ShafaError instance (not raised) for a
    file that failed — FILE_TOO_SMALL below 1 KiB, else the first error in the file's block order.  Other files are unaffected.

    Chain per batch of files (_compress_group, the one copy: compress_files runs it on one file), its length independent of
    the file count: block split (shafa_block_count) -> one unpack_payloads gather into 16-aligned regions when some block
    start is not aligned -> the size pass (rle_encoded_size_dev) over all blocks -> one synchronisation reading every
    block's RLE size; each file's choice is shafa_rle_worthwhile on its block 0 (f.c:250-258) -> rle_encode_tiles over the
    blocks of the files that take RLE only, into regions of exactly the measured sizes, and hist256_tiles over the blocks of
    the plain files only (over all of them with force_freq) -> sf_build_codes + sf_encode_dev over all blocks, RLE and plain
    files mixed (inputs and RLE outputs addressed from one base, tile histograms in one arena) -> the segmented packs, one
    call per kind of file (the single-file packs for a batch of one file) -> one finish.  Two synchronisations per batch.  force_rle keeps the chain without a size pass:
    rle_encode_tiles over all blocks into worst-case regions (2 n + 3, f.c:244), one synchronisation per batch.  Files are
    batched by MANY_GROUP_BLOCKS blocks (_many_files); the RLE encoder cuts its own grids."""
    return _per_group("compress_many", d_in, sizes, block_size, stream, lambda g: _compress_group(g, force_rle, force_freq))


def rle_encoded_sizes(d_in, sizes=None, block_size=65536, stream=None):
    """Will these files take RLE, and how large is each .rle?  The files as compress_many takes them; per file
    (use_rle, [the RLE size of each of its blocks]) — compress_files' choice without force_rle, and the payload sizes its
    .rle.freq would name — or a ShafaError instance (FILE_TOO_SMALL) for a file under 1 KiB.  One read of the data by the
    size pass (rle_encoded_size_dev) and one synchronisation per batch of files; nothing is encoded, and beyond the sizes
    nothing is allocated (block starts that are not 16-aligned are first gathered into aligned regions, as in compress_many)."""
    def body(g):
        r = g.rle_sizes()
        return g.entries(g.errs0, [(u, r[g.first[i]:g.first[i] + g.count[i]]) for i, u in enumerate(g.use_rle(r))])

    return _per_group("rle_encoded_sizes", d_in, sizes, block_size, stream, body)


def shaf_file_bytes(block_sizes):
    """The length of a .shaf file whose blocks have these payload sizes: "@<blocks>", then "@<size>@" + payload per block
    (c.c:351,256-258)."""
    return 1 + len(str(len(block_sizes))) + sum(2 + len(str(int(n))) + int(n) for n in block_sizes)


def compressed_sizes(d_in, sizes=None, block_size=65536, force_rle=False, force_freq=False, stream=None):
    """How large will the files be?  compress_many's arguments and file split; one entry per file: a dict with the keys of
    compress_many's dict for that file, each value the file's length in bytes (an int), or a ShafaError instance with the
    code compress_many's entry has.  No payload byte is written or allocated: the data is read by rle_encoded_hist_dev (the
    RLE histogram and size of every block) and by hist256 (the input's), neither an RLE stream nor a Shannon-Fano stream
    exists.

    Chain per batch of files: the two histogram passes over all blocks -> one synchronisation reading every block's RLE size;
    each file's choice is shafa_rle_worthwhile on its block 0 -> each block's chosen histogram and size picked on the device
    -> sf_build_codes -> sf_encoded_size_dev -> the .cod and .freq texts through the segmented packs (a few KiB a block:
    writing them measures them) -> one finish.  ".rle" is the sum of the file's RLE sizes, ".shaf" shaf_file_bytes of its
    Shannon-Fano sizes.  Two synchronisations per batch, one with force_rle, as compress_many; the same batches
    (_many_files)."""
    return _per_group("compressed_sizes", d_in, sizes, block_size, stream, lambda g: _sizes_group(g, force_rle, force_freq))


def _sizes_group(g, force_rle, force_freq):
    import torch
    bt, st, dev, nb, nf, d_n_in = g.bt, g.st, g.dev, g.nb, g.nf, g.d_n_in
    # ---- Module F's two histograms of every block, without an RLE stream: the choice needs the RLE sizes on the host,
    # and a histogram of the input that ran before it costs no synchronisation of its own
    d_rle_n = torch.zeros(nb, dtype=torch.int64, device=dev)
    d_freq_rle = torch.empty(nb * 256, dtype=torch.int64, device=dev)
    d_freq_in = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
    bt.rle_encoded_hist_dev(st, g.src_in, g.off, g.sizes, d_n_in, d_rle_n, d_freq_rle)
    if force_rle:
        use = [True] * nf
        if force_freq:
            bt.hist256(st, g.src_in, g.off, g.sizes, d_freq_in)
    else:
        bt.hist256(st, g.src_in, g.off, g.sizes, d_freq_in)
        g.errs0 = g.finish()
        use = g.use_rle(_u64_host(d_rle_n))
    # ---- per block: the RLE histogram and size, or the input's
    if all(use):
        e_n, e_freq = d_rle_n, d_freq_rle
    elif not any(use):
        e_n, e_freq = d_n_in, d_freq_in
    else:
        pick = torch.tensor([u for i, u in enumerate(use) for _ in range(g.count[i])], dtype=torch.bool, device=dev)
        with torch.cuda.stream(st):
            e_n = torch.where(pick, d_rle_n, d_n_in)
            e_freq = torch.where(pick.repeat_interleave(256), d_freq_rle, d_freq_in)
    # ---- Module T, and Module C's sizes
    d_tab = torch.empty(nb * C.sizeof(CodeTable), dtype=torch.uint8, device=dev)
    bt.sf_build_codes(st, nb, e_freq, d_tab)
    d_enc_n = torch.zeros(nb, dtype=torch.int64, device=dev)
    bt.sf_encoded_size_dev(st, nb, e_freq, d_tab, d_enc_n)
    # ---- the texts, for their lengths
    modes = [b"R" if u else b"N" for u in use]
    stem = lambda i: ".rle" if use[i] else ""                               # noqa: E731
    g.pack_text("freq", [True] * nf, lambda i: stem(i) + ".freq", modes, e_n, e_freq)
    if force_freq:
        g.pack_text("freq", use, lambda i: ".freq", [b"N"] * nf, d_n_in, d_freq_in)
    g.pack_text("cod", [True] * nf, lambda i: stem(i) + ".cod", modes, e_n, d_tab)
    errs = g.finish()
    rsize, esize = _u64_host(d_rle_n), _u64_host(d_enc_n)
    out = [{key: int(text.numel()) for key, text in files.items()} for files in g.packed()]
    for i in range(nf):
        lo, hi = g.first[i], g.first[i] + g.count[i]
        if use[i]:
            out[i][".rle"] = int(sum(rsize[lo:hi]))
        out[i][stem(i) + ".shaf"] = shaf_file_bytes(esize[lo:hi])
    return g.entries(errs, out)


class _GroupBlocks:
    """One group of files on its device batch (a context manager: leaving it closes the Batch).  The blocks of the files, file
    after file: per block its size (`sizes`; on the device `d_n_in`) and its 16-aligned place (`src_in`, `off`), per file
    (`files`: its index in the call) its first block and block count.  Beside them what every compress driver keeps per
    group: the codes of the size pass (`errs0`), each file's RLE choice, the segmented packs' lengths, keys and buffers, and
    the rule that turns per-block codes into each file's entry."""

    def __init__(self, name, d_in, start, split, files, st):
        import torch
        self.name, self.st, self.dev, self.files, self.nf = name, st, d_in.device, list(files), len(files)
        self.sizes, self.first, self.count, src = [], [], [], []
        for f in files:
            self.first.append(len(self.sizes))
            self.count.append(len(split[f]))
            o = start[f]
            for n in split[f]:
                src.append(o)
                self.sizes.append(n)
                o += n
        self.nb = len(self.sizes)
        self.errs0 = [SUCCESS] * self.nb
        self.lens, self.kinds = None, []                                    # per pack call: (its files, their keys, buffer, offsets)
        self.d_n_in = torch.tensor(self.sizes, dtype=torch.int64, device=self.dev)
        self.bt = Batch(self.nb, 2 * max(self.sizes) + 64)
        self.src_in, self.off = _aligned_blocks(self.bt, st, d_in, src, self.sizes, self.d_n_in)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.bt.close()

    def blocks(self, i):
        return range(self.first[i], self.first[i] + self.count[i])

    def finish(self):
        """one synchronisation -> the per-block codes"""
        return self.bt.finish(self.st, self.nb, raise_on_error=False)[1]

    def rle_sizes(self):
        """The size pass (rle_encoded_size_dev) over every block and its synchronisation, which reads the sizes back -> the RLE
        sizes; its codes stay in errs0"""
        import torch
        d_size = torch.zeros(self.nb, dtype=torch.int64, device=self.dev)
        self.bt.rle_encoded_size_dev(self.st, self.src_in, self.off, self.sizes, self.d_n_in, d_size)
        self.errs0 = self.finish()
        return _u64_host(d_size)

    def use_rle(self, rsize):
        """per file: the reference's decision on its block 0's RLE size (shafa_rle_worthwhile, f.c:250-258)"""
        return [bool(host().shafa_rle_worthwhile(self.sizes[b], rsize[b], False)) for b in self.first]

    def rle_first(self, use, rcap):
        """Put the files that take RLE in front of the plain ones: the blocks of either kind become one range, so each stage
        runs over its range only and a block's error word is the same in every call -> (use, rcap) in the new order"""
        import torch
        order = [i for i in range(self.nf) if use[i]] + [i for i in range(self.nf) if not use[i]]
        if order == list(range(self.nf)):
            return use, rcap
        perm = [b for i in order for b in self.blocks(i)]
        self.files, self.count = [self.files[i] for i in order], [self.count[i] for i in order]
        self.first = [0] + list(itertools.accumulate(self.count))[:-1]
        self.sizes, self.off, self.errs0 = ([v[b] for b in perm] for v in (self.sizes, self.off, self.errs0))
        self.d_n_in = torch.tensor(self.sizes, dtype=torch.int64, device=self.dev)
        return [use[i] for i in order], [rcap[b] for b in perm]

    def _regions(self, sel, keys, bound):
        """For one pack, over the files i with sel[i] under the keys keys(i): a buffer with a 16-aligned region of bound(i)
        bytes per file, and that pack's length words -> (files, buffer, offsets, capacities, lengths), or None without files"""
        import torch
        fs = [i for i in range(self.nf) if sel[i]]
        if not fs:
            return None
        if self.lens is None:                                               # at most five packs: .rle, two .freq, .cod, .shaf
            self.lens = torch.zeros(5 * self.nf, dtype=torch.int64, device=self.dev)
        dcap = [bound(i) for i in fs]
        doff, dtot = _layout(dcap)
        buf = torch.empty(dtot + 16, dtype=torch.uint8, device=self.dev)
        n = self.lens[len(self.kinds) * self.nf:(len(self.kinds) + 1) * self.nf]
        self.kinds.append((fs, [keys(i) for i in fs], buf, doff))
        return fs, buf, doff, dcap, n

    # The packs: segmented, one call per kind of file.  A group of one file takes the single-file pack, which writes the same
    # bytes with one launch and one upload fewer (compress_files pays its fixed cost per call).
    def pack_payloads(self, sel, keys, framing, d_src, src_off, src_cap, d_src_n):
        """the blocks' payloads as .rle (FRAME_RAW) or .shaf (FRAME_SHAF) files, each region sized by pack_payloads_max"""
        r = self._regions(sel, keys, lambda i: pack_payloads_max([src_cap[b] for b in self.blocks(i)], framing))
        if not r:
            return
        fs, buf, doff, dcap, n = r
        if self.nf == 1:
            self.bt.pack_payloads(self.st, framing, d_src, src_off, src_cap, d_src_n, buf, dcap[0], n)
        else:
            self.bt.pack_payloads_files(self.st, [self.first[i] for i in fs], [self.count[i] for i in fs], framing, d_src,
                                        src_off, src_cap, d_src_n, buf, doff, dcap, n)

    def pack_text(self, kind, sel, keys, modes, d_sizes, d_body):
        """.cod (kind "cod", d_body: the code tables) or .freq (kind "freq", d_body: the histograms) files in the files' modes,
        each region sized by pack_cod_max / pack_freq_max"""
        bound = pack_cod_max if kind == "cod" else pack_freq_max
        r = self._regions(sel, keys, lambda i: bound(self.count[i]))
        if not r:
            return
        fs, buf, doff, dcap, n = r
        if self.nf == 1:
            getattr(self.bt, "pack_" + kind)(self.st, self.nb, modes[0], d_sizes, d_body, buf, dcap[0], n)
        else:
            getattr(self.bt, f"pack_{kind}_files")(self.st, [self.first[i] for i in fs], [self.count[i] for i in fs],
                                                   [modes[i] for i in fs], d_sizes, d_body, buf, doff, dcap, n)

    def packed(self):
        """after the finish behind the packs, one read of all lengths -> per file {key: the file, a view of its pack's buffer}"""
        got = self.lens.cpu().tolist()
        out = [{} for _ in range(self.nf)]
        for k, (fs, keys, buf, doff) in enumerate(self.kinds):
            for j, i in enumerate(fs):
                out[i][keys[j]] = buf[doff[j]:doff[j] + got[k * self.nf + j]]
        return out

    def entries(self, errs, out):
        """per file: a ShafaError for its first error in block order, the size pass's (errs0) in front of a later stage's
        (errs), or out[i]"""
        res = []
        for i in range(self.nf):
            lo, hi = self.first[i], self.first[i] + self.count[i]
            b, e = _first_error(self.errs0[lo:hi])
            if not e:
                b, e = _first_error(errs[lo:hi])
            res.append(ShafaError(e, f"{self.name}: block {b}") if e else out[i])
        return res


def _compress_group(g, force_rle, force_freq):
    """compress_many's chain over one group -> its files' entries"""
    import torch
    bt, st, dev, nb, nf = g.bt, g.st, g.dev, g.nb, g.nf
    # ---- the choice per file: forced, or the reference's decision on its block 0's RLE size, measured with every other
    # block's (exact: the encoder fills these regions)
    if force_rle:
        use, rcap = [True] * nf, [2 * n + 3 for n in g.sizes]               # f.c:244
    else:
        rcap = g.rle_sizes()
        use = g.use_rle(rcap)
    use, rcap = g.rle_first(use, rcap)
    src_in, off, sizes, d_n_in = g.src_in, g.off, g.sizes, g.d_n_in
    nr = sum(c for u, c in zip(use, g.count) if u)                            # blocks [0, nr) take RLE, [nr, nb) are plain
    in_lo = 0 if force_freq else nr                                         # the input's histogram: blocks [in_lo, nb)
    # tile histograms: the RLE outputs' then the inputs', in one arena
    th_off, th_tot = _layout([tile_hist_bytes(c) for c in rcap[:nr]] + [tile_hist_bytes(n) for n in sizes[in_lo:]])
    rtoff, itoff = th_off[:nr], [None] * in_lo + th_off[nr:]
    d_th = torch.empty(th_tot + 16, dtype=torch.uint8, device=dev)
    # ---- Module F: RLE over the blocks that take it, into exact regions (worst-case ones with force_rle); the input's
    # histogram over the others
    roff, rtot = _layout(rcap[:nr])
    d_rle = torch.empty(rtot + 16, dtype=torch.uint8, device=dev)
    e_n = d_n_in.clone() if nr else d_n_in                                  # per block: RLE size | input size
    e_freq = torch.zeros(nb * 256, dtype=torch.int64, device=dev)           # per block: RLE histogram | input histogram
    if nr:
        bt.rle_encode_tiles(st, src_in, off[:nr], sizes[:nr], d_rle, roff, rcap[:nr], e_n, e_freq, d_th, rtoff)
    d_freq_in = e_freq
    if in_lo < nb:
        if in_lo < nr:                                                      # force_freq: the RLE files' inputs as well
            d_freq_in = torch.zeros(nb * 256, dtype=torch.int64, device=dev)
            bt.hist256_tiles(st, src_in, off, sizes, d_freq_in, d_th, itoff)
            with torch.cuda.stream(st):
                e_freq[nr * 256:].copy_(d_freq_in[nr * 256:])
        else:
            bt.hist256_tiles(st, src_in, off[nr:], sizes[nr:], e_freq[nr * 256:], d_th, itoff[nr:])
    # ---- Module T and Module C once over all blocks: each block's source and tile histograms by its file
    lo = d_rle if d_rle.data_ptr() < src_in.data_ptr() else src_in          # one base for inputs and RLE outputs
    a_in, a_rle = src_in.data_ptr() - lo.data_ptr(), d_rle.data_ptr() - lo.data_ptr()
    e_off = [a_rle + o for o in roff] + [a_in + o for o in off[nr:]]
    e_cap = rcap[:nr] + sizes[nr:]
    e_toff = rtoff + itoff[nr:]
    d_tab = torch.empty(nb * C.sizeof(CodeTable), dtype=torch.uint8, device=dev)
    bt.sf_build_codes(st, nb, e_freq, d_tab)
    # Fano codes average under H + 1 <= 9 bits a symbol: 12 bits leave room (a block that does not fit is an error)
    ocap = [c + c // 2 + 64 for c in e_cap]
    ooff, otot = _layout(ocap)
    d_enc = torch.empty(otot + 16, dtype=torch.uint8, device=dev)
    d_enc_n = torch.zeros(nb, dtype=torch.int64, device=dev)
    bt.sf_encode_dev(st, lo, e_off, e_cap, e_n, d_tab, d_enc, ooff, ocap, d_enc_n, d_th, e_toff)
    # ---- the files: one pack per kind
    modes = [b"R" if u else b"N" for u in use]
    stem = lambda i: ".rle" if use[i] else ""                               # noqa: E731
    g.pack_payloads(use, lambda i: ".rle", FRAME_RAW, d_rle, roff + [0] * (nb - nr), rcap, e_n)
    g.pack_text("freq", [True] * nf, lambda i: stem(i) + ".freq", modes, e_n, e_freq)
    if force_freq:
        g.pack_text("freq", use, lambda i: ".freq", [b"N"] * nf, d_n_in, d_freq_in)
    g.pack_text("cod", [True] * nf, lambda i: stem(i) + ".cod", modes, e_n, d_tab)
    g.pack_payloads([True] * nf, lambda i: stem(i) + ".shaf", FRAME_SHAF, d_enc, ooff, ocap, d_enc_n)
    errs = g.finish()
    return g.entries(errs, g.packed())


# ------------------------------------------------------------------ files in device memory -> the decoded bytes
UNPACK_INFO_WORDS = 8           # SHAFA_UNPACK_INFO_*: status, mode, count, indexed, framed, largest size
INFO_STATUS, INFO_MODE, INFO_COUNT, INFO_INDEXED, INFO_FRAMED, INFO_MAX_SIZE = range(6)


def unpack_max_blocks(text_n, kind):
    """max_blocks for Batch.unpack_cod ("cod": a parsable block takes >= 258 bytes, "@d@" and 255 ';'), unpack_rle_freq
    ("freq": >= 4 bytes, "@d@x") or unpack_freq ("counts": >= 259 bytes, "@d@", a digit and 255 ';'): a header that announces
    more blocks leaves a failing block among those indexed."""
    return int(text_n) // {"cod": 258, "counts": 259}.get(kind, 4) + 1


def _layout(caps):
    """16-aligned regions of these capacities: (offsets, total bytes)"""
    off, pos = [], 0
    for c in caps:
        off.append(pos)
        pos += _al16(c)
    return off, pos


def _u64_host(t):
    return t.cpu().numpy().view(np.uint64).astype(object).tolist()


def _first_error(errs):
    return next(((i, e) for i, e in enumerate(errs) if e), (len(errs), SUCCESS))


def _rle_measure(bt, st, d_in, in_off, in_n, d_in_n, n_err):
    """The size pass (rle_decoded_size_dev) over these RLE blocks and its synchronisation, which reads the sizes back
    -> (decoded sizes, per-block codes).  n_err: the error words shafa_hipd_finish reads."""
    import torch
    d_size = torch.zeros(max(len(in_n), 1), dtype=torch.int64, device=d_in_n.device)
    bt.rle_decoded_size_dev(st, d_in, in_off, in_n, d_in_n, d_size)
    _, errs = bt.finish(st, n_err, raise_on_error=False)
    return _u64_host(d_size)[:len(in_n)], errs[:len(in_n)]


def _groups(cost, max_bytes):
    """Consecutive blocks whose costs (bytes) fit max_bytes — a block above it is a group of its own -> [(first, end)]"""
    groups, g0, acc = [], 0, 0
    for b, c in enumerate(cost):
        if b > g0 and acc + c > max_bytes:
            groups.append((g0, b))
            g0, acc = b, 0
        acc += c
    groups.append((g0, len(cost)))
    return groups


def _rle_groups(sizes, max_bytes):
    """Consecutive blocks whose exact output regions (_al16(size)) fit max_bytes -> [(first, end)]; rle_decode_dev cuts its
    own grids, however many small blocks join a large one"""
    return _groups([_al16(s) for s in sizes], max_bytes)


def _rle_decode_groups(bt, st, d_in, in_off, in_n, d_in_n, sizes, max_bytes, groups=None):
    """rle_decode_dev of these blocks into regions of exactly their decoded sizes (_rle_measure's), group after group
    (`groups`, or _rle_groups) into one buffer sized for the largest group.  Yields (first, end, buffer, offsets, device
    sizes) once a group's decode is enqueued; what the caller enqueues then reads the buffer before the next group's decode
    overwrites it.  Groups that decode to nothing are left out.  Enqueues only."""
    import torch
    dev = d_in.device
    groups = groups or _rle_groups(sizes, max_bytes)
    biggest = max(_layout(sizes[a:z])[1] for a, z in groups)
    d_out = torch.empty(biggest + 16, dtype=torch.uint8, device=dev)
    d_out_n = torch.zeros(len(sizes), dtype=torch.int64, device=dev)
    for a, z in groups:
        if not sum(sizes[a:z]):
            continue
        off, _ = _layout(sizes[a:z])
        bt.rle_decode_dev(st, d_in, in_off[a:z], in_n[a:z], d_in_n[a:z], d_out, off, sizes[a:z], d_out_n[a:z])
        yield a, z, d_out, off, d_out_n[a:z]


def _rle_decode_exact(bt, st, d_in, in_off, in_n, d_in_n, sizes, max_bytes):
    """_rle_decode_groups, each group packed into its place in one tensor of exactly the decoded bytes -> that tensor; the
    groups follow each other on the stream without a synchronisation.  Enqueues only: the caller's finish ends it."""
    import torch
    dev = d_in.device
    d_len = torch.zeros(max(len(sizes), 1), dtype=torch.int64, device=dev)       # a group's length, at its first block
    total = sum(sizes)
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    pos = 0
    for a, z, d_out, off, d_out_n in _rle_decode_groups(bt, st, d_in, in_off, in_n, d_in_n, sizes, max_bytes):
        gt = sum(sizes[a:z])
        bt.pack_payloads(st, FRAME_RAW, d_out, off, sizes[a:z], d_out_n, out[pos:], gt, d_len[a:a + 1])
        pos += gt
    return out[:total]


def _decode_args(shaf, cod, rle, freq, what):
    """decompress_files' argument checks -> (sf, [payload file, text file])"""
    import torch
    sf = shaf is not None or cod is not None
    if sf and (shaf is None or cod is None or rle is not None or freq is not None):
        raise ValueError(f"{what}: shaf and cod go together, without rle / freq")
    if not sf and (rle is None or freq is None):
        raise ValueError(f"{what}: give shaf and cod, or rle and freq")
    files = [t.reshape(-1) for t in ((shaf, cod) if sf else (rle, freq))]
    for t in files:
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{what}: files are contiguous uint8 CUDA tensors")
    return sf, files


def _accepted_modes(sf, decode_rle):
    """The modes a decode takes from the .cod or .freq.  decode_rle True asks for RLE bytes to decode: mode R only; False, and
    None ("as the .cod's mode says"), take a .shaf + .cod of either mode."""
    return "RN" if sf and not decode_rle else "R"


def _no_rle_stage(sf, mode, decode_rle):
    """whether the decoded bytes are the SF decoder's output: a mode-N pair, or a mode-R pair read as its .rle bytes"""
    return sf and (mode == "N" or decode_rle is False)


def _parse_rules(what, info, errs, pn, nsym, sf, modes):
    """The rules behind the parse's synchronisation, for one file, on plain lists: its info words, and from its first slot
    on the per-block codes, payload sizes and (sf) symbol counts -> (mode, fb, perr): the blocks in front of the first parse
    fault, and that fault.  Raises a bad header, a mode outside `modes` and a fault on block 0; fb == 0 without one is the
    empty file.  A symbol count above 8 x the payload's bytes is a fault of that block (decompress_files)."""
    if info[INFO_STATUS]:
        raise ShafaError(FILE_STREAM_FAILED, f"{what}: bad header")
    mode = chr(info[INFO_MODE])
    if mode not in modes:
        raise ShafaError(FILE_UNRECOGNIZABLE, f"{what}: mode {mode!r}")
    nidx = info[INFO_INDEXED]
    errs = errs[:nidx]
    if sf:
        errs = [e if e or nsym[b] <= 8 * pn[b] else FILE_UNRECOGNIZABLE for b, e in enumerate(errs)]
    fb, perr = _first_error(errs)
    if not perr and info[INFO_COUNT] > nidx:                                 # cannot happen: max_blocks covers any count
        perr = FILE_STREAM_FAILED
    if fb == 0 and perr:
        raise ShafaError(perr, f"{what}: block 0")
    return mode, fb, perr


def _sf_decode_again(bt, st, args, errs, lo, hi, again, width):
    """While the first error of blocks [lo, hi) of an sf_decode_dev call (`args`: what followed its stream; errs: its codes) is
    LACK_OF_MEMORY at a block not yet in `again` — the decoder's one slot for 33..64-bit codes was taken by another block —
    that block is decoded again on its own: one synchronisation each, over `width` error words; its code in errs is replaced
    and it joins `again`.  -> the span's first error now, as (block - lo, code)"""
    d_pay, poff, pn, d_n, d_tab, d_nsym, d_sfo, ooff, nsym = args
    tsz = C.sizeof(CodeTable)
    b, e = _first_error(errs[lo:hi])
    while e == LACK_OF_MEMORY and lo + b not in again:
        g = lo + b
        bt.sf_decode_dev(st, d_pay, poff[g:g + 1], pn[g:g + 1], d_n[g:g + 1], d_tab[g * tsz:(g + 1) * tsz], d_nsym[g:g + 1],
                         d_sfo, ooff[g:g + 1], nsym[g:g + 1])
        _, one = bt.finish(st, width, raise_on_error=False)
        errs[g] = one[0]
        again.add(g)
        b, e = _first_error(errs[lo:hi])
    return b, e


class _ParsedSet:
    """One file set on its batch, for the single-set decode drivers (the decode side's _GroupBlocks).  Making it checks the
    file arguments (decompress_files') and takes the stream; entering it opens the Batch — closed on leaving — and parses:
    unpack_cod + unpack_shaf (or unpack_rle_freq), one synchronisation, 16 bytes a block read back, _parse_rules.  Then it
    holds mode; fb, the blocks in front of the first parse fault, with their payload sizes (pn) and symbol counts (nsym, .cod
    only); perr, that fault, which fault() raises at the driver's place for it; plain, whether the decoded bytes are the SF
    decoder's output (_no_rle_stage); the device arrays of the parse; max_bytes (default: a quarter of the free device
    memory).  decode_rle: the caller's True or False, or None for "as the .cod's mode says"."""

    def __init__(self, what, shaf, cod, rle, freq, stream, max_bytes=None, decode_rle=None):
        self.what, self.max_bytes = what, max_bytes
        self.decode_rle = decode_rle if decode_rle is None else bool(decode_rle)
        self.sf, self.files = _decode_args(shaf, cod, rle, freq, what)
        self.dev = self.files[0].device
        self.st = _stream(self.dev, stream)
        self.mb = unpack_max_blocks(self.files[1].numel(), "cod" if self.sf else "freq")
        if self.mb > 0x7FFFFFFF:
            raise ShafaError(LACK_OF_MEMORY, f"{what}: text too long")

    def __enter__(self):
        self.bt = Batch(self.mb, 1 << 20)
        try:
            self.max_bytes = _max_bytes(self.dev, self.max_bytes)
            self._parse()
        except BaseException:
            self.bt.close()
            raise
        return self

    def __exit__(self, *exc):
        self.bt.close()

    def _parse(self):
        import torch
        bt, st, sf, files, mb, dev = self.bt, self.st, self.sf, self.files, self.mb, self.dev
        d_info = torch.zeros(UNPACK_INFO_WORDS, dtype=torch.int64, device=dev)
        self.d_off = torch.zeros(mb, dtype=torch.int64, device=dev)
        self.d_n = torch.zeros(mb, dtype=torch.int64, device=dev)
        if sf:
            self.d_nsym = torch.zeros(mb, dtype=torch.int64, device=dev)
            self.d_tab = torch.empty(mb * C.sizeof(CodeTable), dtype=torch.uint8, device=dev)
            bt.unpack_cod(st, mb, files[1], d_info, self.d_nsym, self.d_tab)
            bt.unpack_shaf(st, mb, files[0], d_info[INFO_INDEXED:INFO_INDEXED + 1], self.d_off, self.d_n)
        else:
            bt.unpack_rle_freq(st, mb, files[1], files[0].numel(), d_info, self.d_off, self.d_n)
        _, errs = bt.finish(st, mb, raise_on_error=False)                    # the parse's one synchronisation
        info = _u64_host(d_info)
        pn = _u64_host(self.d_n)[:info[INFO_INDEXED]]
        nsym = _u64_host(self.d_nsym)[:info[INFO_INDEXED]] if sf else None
        self.mode, self.fb, self.perr = _parse_rules(self.what, info, errs, pn, nsym, sf, _accepted_modes(sf, self.decode_rle))
        self.pn, self.nsym = pn[:self.fb], nsym[:self.fb] if sf else None
        self.plain = _no_rle_stage(sf, self.mode, self.decode_rle)

    def fault(self):
        """raises the parse fault, if there is one: each driver calls this where that fault comes in its order of errors"""
        if self.perr:
            raise ShafaError(self.perr, f"{self.what}: block {self.fb}")

    def check(self, errs, b0=0):
        """raises the first of these per-block codes, of blocks b0 on, in block order"""
        b, e = _first_error(errs)
        if e:
            raise ShafaError(e, f"{self.what}: block {b0 + b}")

    def finish_rle(self):
        """the synchronisation behind rle_decode_dev of measured blocks, with the late rule: the size pass accepted every
        block, so an error now is the device's and names no block"""
        _, errs = self.bt.finish(self.st, self.bt.max_blocks, raise_on_error=False)
        _, e = _first_error(errs)
        if e:
            raise ShafaError(e, f"{self.what}: RLE decoding")

    def gather(self, b0, b1):
        """unpack_payloads of blocks [b0, b1) into exact aligned regions -> (buffer, offsets, sizes, device sizes)"""
        import torch
        pn = self.pn[b0:b1]
        poff, ptot = _layout(pn)
        d_pay = torch.empty(ptot + 16, dtype=torch.uint8, device=self.dev)
        self.bt.unpack_payloads(self.st, self.files[0], self.d_off[b0:b1], self.d_n[b0:b1], d_pay, poff, pn)
        return d_pay, poff, pn, self.d_n[b0:b1]

    def sf_decode(self, b0, b1, pack, then=None):
        """Blocks [b0, b1) of a .shaf / .cod pair: unpack_payloads -> sf_decode_dev (-> pack_payloads(RAW) when `pack`; ->
        then(buffer, offsets, sizes, device sizes), which enqueues a reader of the decoded regions, when given) -> one
        synchronisation; a block whose codes take the decoder's single slot for 33..64-bit codes from another is decoded
        again on its own (_sf_decode_again; the pack and `then` run again).  The first SF error in block order raises.
        -> (buffer, offsets, sizes, device sizes) of the decoded blocks, and the packed tensor (None without `pack`)"""
        import torch
        bt, st, dev = self.bt, self.st, self.dev
        tsz = C.sizeof(CodeTable)
        d_pay, poff, pn, d_n = self.gather(b0, b1)
        nsym, d_nsym = self.nsym[b0:b1], self.d_nsym[b0:b1]
        ooff, otot = _layout(nsym)
        d_sfo = torch.empty(otot + 16, dtype=torch.uint8, device=dev)
        args = (d_pay, poff, pn, d_n, self.d_tab[b0 * tsz:b1 * tsz], d_nsym, d_sfo, ooff, nsym)
        bt.sf_decode_dev(st, *args)
        out = None
        if pack:
            total = sum(nsym)
            out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
            d_len = torch.zeros(1, dtype=torch.int64, device=dev)
            bt.pack_payloads(st, FRAME_RAW, d_sfo, ooff, nsym, d_nsym, out, total, d_len)
        if then:
            then(d_sfo, ooff, nsym, d_nsym)
        _, errs = bt.finish(st, bt.max_blocks, raise_on_error=False)
        errs = errs[:b1 - b0]
        again = set()
        _sf_decode_again(bt, st, args, errs, 0, b1 - b0, again, bt.max_blocks)
        self.check(errs, b0)
        if again and (pack or then):
            if pack:
                bt.pack_payloads(st, FRAME_RAW, d_sfo, ooff, nsym, d_nsym, out, total, d_len)
            if then:
                then(d_sfo, ooff, nsym, d_nsym)
            bt.finish(st, bt.max_blocks)
        return (d_sfo, ooff, nsym, d_nsym), (out[:total] if pack else None)

    def measure(self):
        """The decoded size of every block in front of the first parse fault (fb > 0), and the RLE decoder's inputs (buffer,
        offsets, sizes, device sizes; None for a plain set, whose sizes are the .cod's).  An RLE set goes through
        unpack_payloads (and sf_decode_dev for .shaf + .cod) and the size pass; the first SF error, then the first RLE error
        in block order raise."""
        if self.plain:
            return list(self.nsym), None
        rin = self.sf_decode(0, self.fb, False)[0] if self.sf else self.gather(0, self.fb)
        sizes, errs = _rle_measure(self.bt, self.st, *rin, self.bt.max_blocks)
        self.check(errs)
        return sizes, rin

    def rle_range(self, rin, sizes, b0, b1):
        """blocks [b0, b1) of a measured RLE set, decoded and packed -> their bytes; synchronised"""
        d_in, in_off, in_n, d_in_n = rin
        out = _rle_decode_exact(self.bt, self.st, d_in, in_off[b0:b1], in_n[b0:b1], d_in_n[b0:b1], sizes[b0:b1], self.max_bytes)
        self.finish_rle()
        return out

    def plan(self, measured=True):
        """What walk goes by (fb > 0), settled before anything of the groups is enqueued: `sizes` of the regions a reader is
        given, block by block, `starts` (their prefix sums) and `groups`, [(first, end)] within max_bytes.
          a plain set                      the .cod's symbol counts; groups by _al16(symbols) + _al16(payload)
          an RLE form, measured            measure(), then the parse fault; the decoded sizes; _rle_groups
          an RLE form, measured=False      its RLE bytes as they leave the SF decoder (or lie in the .rle), grouped as a plain
                                           set (.rle: by _al16(payload)): build_index, whose entry measures them itself"""
        import itertools
        self.rin = None
        if self.plain or not measured:
            self.sizes = list(self.nsym if self.sf else self.pn)
            cost = [_al16(s) + _al16(n) for s, n in zip(self.sizes, self.pn)] if self.sf else [_al16(n) for n in self.pn]
            self.groups = _groups(cost, self.max_bytes)
        else:
            self.sizes, self.rin = self.measure()
            self.fault()
            self.groups = _rle_groups(self.sizes, self.max_bytes)
        self.starts = list(itertools.accumulate(self.sizes, initial=0))

    def walk(self, reader, before_last=None):
        """The blocks of a planned set, group by group: reader(a, z, buffer, offsets, sizes, device sizes) enqueues what reads
        the regions of blocks [a, z), which hold until the next group is decoded.  A reader may be called a second time for
        the same group — a block of it was decoded again (sf_decode) — and must then leave what a single call would have left;
        that is all the walk promises about calls.  before_last() is enqueued behind the last group's reader, in front of the
        last synchronisation.
          a plain set            sf_decode -> reader, one synchronisation a group, which raises the group's SF faults; the parse
                                 fault behind the last group
          an unmeasured RLE form sf_decode and its synchronisation (.rle: unpack_payloads) -> reader -> one synchronisation a
                                 group; the reader's per-block codes wait for the SF faults of the groups behind, then raise in
                                 block order; then the parse fault
          a measured RLE form    rle_decode_dev -> reader, the groups back to back on the stream through one reused buffer
                                 (_rle_decode_groups; groups that decode to nothing are left out), one synchronisation
                                 (finish_rle)"""
        bt, st = self.bt, self.st
        if self.rin is not None:
            for a, z, d_a, a_off, d_a_n in _rle_decode_groups(bt, st, *self.rin, self.sizes, self.max_bytes, self.groups):
                reader(a, z, d_a, a_off, self.sizes[a:z], d_a_n)
            if before_last:
                before_last()
            return self.finish_rle()
        codes = []
        for a, z in self.groups:
            def then(*regions):
                reader(a, z, *regions)
                if before_last and z == self.fb:
                    before_last()
            if self.plain:                                                   # no fault of its own: within the group's one synchronisation
                self.sf_decode(a, z, False, then)
                continue
            then(*(self.sf_decode(a, z, False)[0] if self.sf else self.gather(a, z)))
            _, errs = bt.finish(st, bt.max_blocks, raise_on_error=False)
            codes += errs[:z - a]
        self.check(codes)
        self.fault()


def decompress_files(shaf=None, cod=None, rle=None, freq=None, decode_rle=True, stream=None, max_bytes=None):
    """The file the CLI's Module D writes, decoded from files held in device memory (contiguous uint8 CUDA tensors, any
    alignment — e.g. compress_files' values):
      shaf + cod, decode_rle=False   `shafa X.shaf -m d`, or `X.rle.shaf -m d -d s` (the .rle bytes)
      shaf + cod, decode_rle=True    `shafa X.rle.shaf` (a mode-N .cod is SHAFA_FILE_UNRECOGNIZABLE, d.c:678)
      rle + freq                     `shafa X.rle -m d` (the .freq's mode must be R)
    Returns a uint8 CUDA tensor holding exactly the decoded file.  Errors raise ShafaError(code): the first error in block
    order, which is the C host's on files with one fault (include/shafa_hip.h: "Files in device memory, parsed").

    Chain: unpack_cod + unpack_shaf (or unpack_rle_freq) -> one synchronisation, 16 bytes a block read back -> exact
    aligned regions -> unpack_payloads -> sf_decode_dev -> pack_payloads -> finish: two synchronisations without RLE
    decoding.  RLE decoding first measures every block (rle_decoded_size_dev, one synchronisation that reads the sizes),
    then decodes into regions of exactly those sizes, in groups that fit max_bytes (default: a quarter of the free device
    memory) and follow each other without a synchronisation, each packed into its place in the result; one last
    synchronisation.  A symbol count above 8 x the payload's bytes is SHAFA_FILE_UNRECOGNIZABLE without
    decoding (every code of a table the decoder accepts has >= 1 bit, so the host's decoder runs out of input).  A block whose
    codes take the decoder's single slot for 33..64-bit codes from another is decoded again on its own."""
    import torch
    with _ParsedSet("decompress_files", shaf, cod, rle, freq, stream, max_bytes, decode_rle) as s:
        if s.fb == 0:
            return torch.empty(0, dtype=torch.uint8, device=s.dev)
        if s.plain:
            _, out = s.sf_decode(0, s.fb, not s.perr)
            s.fault()
            return out
        sizes, rin = s.measure()
        s.fault()
        return s.rle_range(rin, sizes, 0, s.fb)


def decoded_sizes(shaf=None, cod=None, rle=None, freq=None, stream=None):
    """The decoded size of every block of a file set held in device memory (decompress_files' file arguments), as a list of
    ints whose sum is the decoded file's length — the original file's: a mode-R .shaf + .cod counts its blocks after RLE
    decoding, a mode-N pair is what decompress_files(decode_rle=False) returns.  Nothing is decoded that need not be:
      shaf + cod, mode N   the .cod's block sizes; the .shaf is framed (unpack_shaf), no payload is read
      rle + freq           unpack_payloads and the size pass (rle_decoded_size_dev)
      shaf + cod, mode R   unpack_payloads, sf_decode_dev, then the size pass on the RLE bytes; no RLE output is allocated
    Raises what decompress_files raises for faults in what the call looked at, with its precedence: header, mode, parse
    faults, and for the two RLE forms the SF and RLE faults of every block."""
    with _ParsedSet("decoded_sizes", shaf, cod, rle, freq, stream, 0) as s:  # no working memory to bound: nothing is asked
        sizes = s.measure()[0] if s.fb else []
        s.fault()
        return [int(n) for n in sizes]


def decompress_range(offset, length, shaf=None, cod=None, rle=None, freq=None, stream=None, max_bytes=None):
    """Bytes [offset, offset + length) of the decoded file of a file set held in device memory: a uint8 CUDA tensor equal to
    the same slice of decompress_files' result (decode_rle following the .cod's mode, as in decoded_sizes; Python slice
    semantics at the end of the file; a negative offset or length raises ValueError).
    Block-granular: the per-block sizes as in decoded_sizes, a prefix sum on the host, the blocks [b0, b1) that cover the
    range, and only those go through the expensive stage — mode N: unpack_payloads and sf_decode_dev of blocks b0 .. b1 - 1
    only; rle + freq: rle_decode_dev of those only; mode-R shaf + cod: every block is SF-decoded (the sizes need it), only the
    covering ones are RLE-decoded.  Then one pack_payloads(RAW) and a slice (a view of the covering blocks' bytes).
    Errors: parse faults anywhere in the files, and decode faults in every block the call decoded or measured, raise with
    decompress_files' code and precedence; a damaged payload in a mode-N block outside the range is, by design, not noticed."""
    import bisect
    import itertools
    import torch
    what = "decompress_range"
    if offset < 0 or length < 0:
        raise ValueError(f"{what}: negative offset or length")
    with _ParsedSet(what, shaf, cod, rle, freq, stream, max_bytes) as s:
        out, lo, hi = torch.empty(0, dtype=torch.uint8, device=s.dev), 0, 0
        if s.fb:
            sizes, rin = s.measure()
            ends = list(itertools.accumulate(sizes))                         # block b is bytes [ends[b] - sizes[b], ends[b])
            lo, hi = min(offset, ends[-1]), min(offset + length, ends[-1])
            if lo < hi:
                b0, b1 = bisect.bisect_right(ends, lo), bisect.bisect_left(ends, hi) + 1
                out = s.sf_decode(b0, b1, True)[1] if rin is None else s.rle_range(rin, sizes, b0, b1)
                first = ends[b0] - sizes[b0]
                lo, hi = lo - first, hi - first
        s.fault()
        return out[lo:hi]


Verify = collections.namedtuple("Verify", "equal first_diff decoded_size")


def _ref_spans(sizes, ref_len):
    """What each of these decoded blocks, laid end to end, is compared with in an original of ref_len bytes: (offsets,
    sizes) — a block that starts at or behind the original's end with no byte, one that straddles it with what remains"""
    off, n, pos = [], [], 0
    for s in sizes:
        o = min(pos, ref_len)
        off.append(o)
        n.append(min(s, ref_len - o))
        pos += s
    return off, n


def verify_files(d_in, shaf=None, cod=None, rle=None, freq=None, decode_rle=True, stream=None, max_bytes=None):
    """Whether a file set held in device memory (decompress_files' file arguments and decode_rle) still decodes to d_in, a
    contiguous uint8 CUDA tensor on the files' device (any alignment, may be empty) -> Verify(equal, first_diff,
    decoded_size).  With out = decompress_files(the same files): decoded_size = out.numel(); equal = the two are the same
    bytes; first_diff = None when equal, else the smallest index at which they differ, or the smaller length when one is a
    prefix of the other.  Raises what decompress_files raises: every block is decoded, so faults come before any difference,
    wherever it lies.
    Neither the decoded file nor a copy of d_in ever exists: blocks are decoded in groups that fit max_bytes (default: a
    quarter of the free device memory) into exact aligned regions, which compare_dev reads against d_in in place.
    The chain is _ParsedSet.walk's with compare_dev as the reader:
      shaf + cod, mode N (decode_rle=False)   groups by _al16(symbols) + _al16(payload); each runs unpack_payloads ->
                                  sf_decode_dev -> compare_dev -> one synchronisation
      rle + freq; shaf + cod, mode R          the measure as in decompress_files (a mode-R set keeps its .rle bytes resident),
                                  then per group of _rle_groups rle_decode_dev -> compare_dev into one reused buffer, back to
                                  back on the stream; one synchronisation ends the call
    The results are read once, behind the last synchronisation.  No pack_payloads(RAW) runs.  A mode-R .cod with
    decode_rle=False is compared as the .rle bytes, group by group as mode N."""
    import torch
    what = "verify_files"
    s = _ParsedSet(what, shaf, cod, rle, freq, stream, max_bytes, decode_rle)
    if not isinstance(d_in, torch.Tensor) or d_in.dtype != torch.uint8 or not d_in.is_contiguous() or d_in.device != s.dev:
        raise ValueError(f"{what}: d_in is a contiguous uint8 CUDA tensor on the files' device")
    d_in = d_in.reshape(-1)
    ref_len = d_in.numel()
    with s:
        sizes, ref_n, first = [], [], []
        if s.fb:
            s.plan()
            sizes = s.sizes
            ref_off, ref_n = _ref_spans(sizes, ref_len)
            d_first = torch.zeros(s.fb, dtype=torch.int64, device=s.dev)

            def compare(a, z, d_a, a_off, a_cap, d_a_n):
                s.bt.compare_dev(s.st, d_a, a_off, a_cap, d_a_n, d_in if ref_len else d_a, ref_off[a:z], ref_n[a:z], d_first[a:z])
            s.walk(compare)
            first = _u64_host(d_first)
        # the first block that is not its span of d_in; behind the last one d_in may go on
        pos = 0
        for n, r, f in zip(sizes, ref_n, first):
            if f < n or r != n:
                return Verify(False, pos + f, sum(sizes))
            pos += n
        return Verify(ref_len == pos, None if ref_len == pos else pos, pos)


# ------------------------------------------------------------------ CRC-32
_CRC_POLY = 0xEDB88320


def _crc_mul(a, b):
    """a b mod P; a 32-bit value is a polynomial over GF(2), bit 31 = x^0 (the reflected form of zlib's register)"""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ _CRC_POLY if b & 1 else b >> 1
    return p


def _crc_x_pow(e):
    """x^e mod P"""
    r, s = 0x80000000, 0x40000000
    while e:
        if e & 1:
            r = _crc_mul(r, s)
        s = _crc_mul(s, s)
        e >>= 1
    return r


def crc32_combine(crc1, crc2, len2):
    """zlib.crc32(A + B) from crc1 = zlib.crc32(A), crc2 = zlib.crc32(B) and len2 = len(B): crc1 x^(8 len2) mod P ^ crc2, on
    finished values (zlib's crc32_combine).  Plain integers, no device; len2 of any size.  Associative, so per-part digests
    join in any grouping; Batch.crc32_combine_dev is the same rule on device arrays."""
    if len2 < 0:
        raise ValueError("crc32_combine: negative length")
    return _crc_mul(_crc_x_pow(8 * int(len2) % 0xFFFFFFFF), int(crc1) & 0xFFFFFFFF) ^ (int(crc2) & 0xFFFFFFFF)


CRC_PIECE = 1 << 26             # crc32: a segment is digested in pieces of 64 MiB (8192 tiles: 2^18 pieces stay below 2^31 tiles)
Checksum = collections.namedtuple("Checksum", "crc32 decoded_size")


def crc32(d_in, sizes=None, stream=None, _piece=None):
    """zlib.crc32 of a contiguous uint8 CUDA tensor, digested where it lies (any alignment, nothing is copied) -> int.  With
    `sizes`: of each of the consecutive segments of these lengths (compress_many's convention, the segments at whatever
    alignment they fall) -> a list of ints.  An empty tensor or segment gives 0.
    A segment longer than CRC_PIECE (64 MiB) is cut into pieces of that size, one block each for crc32_dev, and the pieces'
    CRCs are joined by crc32_combine_dev; a call of crc32_dev takes at most 2^17 pieces (2^30 tiles).  One synchronisation,
    which reads 4 bytes per segment."""
    import torch
    if not isinstance(d_in, torch.Tensor) or d_in.dtype != torch.uint8 or not d_in.is_cuda or not d_in.is_contiguous():
        raise ValueError("crc32: d_in is a contiguous uint8 CUDA tensor")
    d_in = d_in.reshape(-1)
    segs = [int(d_in.numel())] if sizes is None else [int(n) for n in sizes]
    if any(n < 0 for n in segs) or sum(segs) > d_in.numel():
        raise ValueError("crc32: sizes exceed d_in")
    piece = int(_piece) if _piece else CRC_PIECE
    off, cap, first, count, pos = [], [], [], [], 0
    for n in segs:
        first.append(len(off))
        for a in range(0, n, piece):
            off.append(pos + a)
            cap.append(min(piece, n - a))
        count.append(len(off) - first[-1])
        pos += n
    out = [0] * len(segs)
    if off:
        dev = d_in.device
        st = _stream(dev, stream)
        bt = Batch(max(len(off), len(segs)), piece)
        try:
            d_n = torch.tensor(cap, dtype=torch.int64).to(dev)
            d_crc = torch.zeros(len(off), dtype=torch.int32, device=dev)
            d_file_crc = torch.zeros(len(segs), dtype=torch.int32, device=dev)
            d_file_n = torch.zeros(len(segs), dtype=torch.int64, device=dev)
            calls = max(1, (1 << 30) // max(1, -(-piece // 8192)))           # pieces per crc32_dev call
            for a in range(0, len(off), calls):
                z = min(a + calls, len(off))
                bt.crc32_dev(st, d_in, off[a:z], cap[a:z], d_n[a:z], d_crc[a:z])
            bt.crc32_combine_dev(st, first, count, d_crc, d_n, d_file_crc, d_file_n)
            bt.finish(st, len(off))
            out = [int(c) & 0xFFFFFFFF for c in d_file_crc.cpu().tolist()]
        finally:
            bt.close()
    return out[0] if sizes is None else out


def checksum_files(shaf=None, cod=None, rle=None, freq=None, decode_rle=True, stream=None, max_bytes=None):
    """The CRC-32 and the length of the file a file set held in device memory decodes to (decompress_files' file arguments
    and decode_rle) -> Checksum(crc32, decoded_size).  With out = decompress_files(the same arguments): decoded_size =
    out.numel(), crc32 = zlib.crc32 of out's bytes; raises what that call raises — every block is decoded, so a fault is
    reported whichever group it lies in.  The original need not exist any more: a digest taken from it (shafa.crc32, or
    zlib.crc32 on any host) is what the answer is checked against.
    The decoded file never exists, nor a tensor of its size: verify_files' chain (_ParsedSet.walk, groups that fit max_bytes,
    default a quarter of the free device memory) with crc32_dev where compare_dev is; the combine goes in front of the last
    synchronisation — the last group's for mode N (decode_rle=False), the one that ends the call for the two RLE forms.
    The blocks' CRCs (4 bytes a block) and their device-resident decoded sizes gather on the device; one crc32_combine_dev
    over all blocks ends the call.  No pack_payloads(RAW) runs; the synchronisations are verify_files'."""
    import torch
    with _ParsedSet("checksum_files", shaf, cod, rle, freq, stream, max_bytes, decode_rle) as s:
        if s.fb == 0:
            return Checksum(0, 0)
        bt, st, dev = s.bt, s.st, s.dev
        s.plan()
        d_crc = torch.zeros(s.fb, dtype=torch.int32, device=dev)
        d_file_crc = torch.zeros(1, dtype=torch.int32, device=dev)
        d_file_n = torch.zeros(1, dtype=torch.int64, device=dev)
        # the decoded sizes on the device: the .cod's, or the RLE decoder's own, gathered group by group
        d_n = s.d_nsym[:s.fb] if s.plain else torch.zeros(s.fb, dtype=torch.int64, device=dev)

        def digest(a, z, d_a, a_off, a_cap, d_a_n):
            bt.crc32_dev(st, d_a, a_off, a_cap, d_a_n, d_crc[a:z])
            if not s.plain:
                with torch.cuda.stream(st):
                    d_n[a:z].copy_(d_a_n)

        # the combine: behind every group's CRCs on the stream
        s.walk(digest, lambda: bt.crc32_combine_dev(st, [0], [s.fb], d_crc, d_n, d_file_crc, d_file_n))
        return Checksum(int(d_file_crc.cpu()[0]) & 0xFFFFFFFF, int(d_file_n.cpu()[0]))


# ------------------------------------------------------------------ pattern search
FIND_NEXT, FIND_CONTEXT, FIND_MAX_PATTERN = 1, 2, 256
FIND_PIECE = 1 << 26            # find: a segment is searched in chained pieces of 64 MiB (8192 tiles each)
Found = collections.namedtuple("Found", "count positions size")


def _find_args(pattern, max_hits, what):
    """the pattern as bytes and max_hits as an int, or ValueError"""
    try:
        pat = memoryview(pattern).tobytes()
    except TypeError:
        raise ValueError(f"{what}: pattern is bytes-like") from None
    if not 1 <= len(pat) <= FIND_MAX_PATTERN:
        raise ValueError(f"{what}: pattern of 1 .. {FIND_MAX_PATTERN} bytes")
    try:
        hits = -1 if isinstance(max_hits, bool) else max_hits.__index__()
    except (AttributeError, TypeError):
        hits = -1
    if hits < 0:
        raise ValueError(f"{what}: max_hits is a non-negative int")
    return pat, hits


def find(d_in, pattern, sizes=None, max_hits=65536, stream=None, _piece=None):
    """Where `pattern` (bytes-like, 1 .. 256 bytes) occurs in a contiguous uint8 CUDA tensor, searched where it lies (any
    alignment, nothing is copied) -> Found(count, positions, size): count = the number of occurrences, overlapping ones
    included (exact, however small max_hits is), positions = the first min(count, max_hits) of them as an ascending numpy
    int64 array of indices into the tensor, size = the bytes searched.  With `sizes` (crc32's convention): each of the
    consecutive segments of these lengths is searched on its own — an occurrence that straddles two segments is none — and
    the call returns a list of Found, positions relative to the segment, max_hits per segment.
    A segment longer than FIND_PIECE (64 MiB) is cut into pieces of that size, one region each for find_dev, chained with
    FIND_NEXT, so an occurrence over a piece seam is found.  With max_hits = 0 all segments go through one find_dev call
    and the counts are the regions'; else one call per segment appends into the segment's own part of one array (at most
    min(max_hits, size - len(pattern) + 1) entries: a segment has no more occurrences).  One synchronisation, then the
    counts and the positions kept are read."""
    import itertools
    import torch
    if not isinstance(d_in, torch.Tensor) or d_in.dtype != torch.uint8 or not d_in.is_cuda or not d_in.is_contiguous():
        raise ValueError("find: d_in is a contiguous uint8 CUDA tensor")
    pat, max_hits = _find_args(pattern, max_hits, "find")
    d_in = d_in.reshape(-1)
    segs = [int(d_in.numel())] if sizes is None else [int(n) for n in sizes]
    if any(n < 0 for n in segs) or sum(segs) > d_in.numel():
        raise ValueError("find: sizes exceed d_in")
    piece = int(_piece) if _piece else FIND_PIECE
    m = len(pat)
    off, cap, flags, pos, first, start = [], [], [], [], [], 0
    for n in segs:
        first.append(len(off))
        for a in range(0, n, piece):
            off.append(start + a)
            cap.append(min(piece, n - a))
            pos.append(a)
            flags.append(FIND_NEXT if a + piece < n else 0)
        start += n
    first.append(len(off))
    counts, kept, hoff, h = [0] * len(segs), [0] * len(segs), [0] * len(segs), np.empty(0, dtype=np.int64)
    if off:
        dev = d_in.device
        st = _stream(dev, stream)
        bt = Batch(len(off), piece)
        try:
            d_n = torch.tensor(cap, dtype=torch.int64).to(dev)
            d_count = torch.zeros(len(off), dtype=torch.int64, device=dev)
            d_total = torch.zeros(len(segs), dtype=torch.int64, device=dev)
            if max_hits == 0:
                bt.find_dev(st, d_in, off, cap, d_n, flags, pos, pat, 0, None, d_count, d_total)
                bt.finish(st, len(off))
                c = d_count.cpu().tolist()
                counts = [sum(c[a:z]) for a, z in zip(first, first[1:])]
            else:
                room = [min(max_hits, max(0, n - m + 1)) for n in segs]
                hoff = list(itertools.accumulate(room, initial=0))
                d_hits = torch.empty(max(hoff[-1], 1), dtype=torch.int64, device=dev)
                for i, (a, z) in enumerate(zip(first, first[1:])):
                    if a < z:
                        bt.find_dev(st, d_in, off[a:z], cap[a:z], d_n[a:z], flags[a:z], pos[a:z], pat, room[i],
                                    d_hits[hoff[i]:] if room[i] else None, d_count[a:z], d_total[i:i + 1])
                bt.finish(st, len(off))
                counts = d_total.cpu().tolist()
                kept = [min(c, r) for c, r in zip(counts, room)]
                h = d_hits[:max((o + k for o, k in zip(hoff, kept) if k), default=0)].cpu().numpy()
        finally:
            bt.close()
    out = [Found(int(c), h[o:o + k].copy(), n) for c, k, o, n in zip(counts, kept, hoff, segs)]
    return out[0] if sizes is None else out


def find_files(pattern, shaf=None, cod=None, rle=None, freq=None, decode_rle=True, max_hits=65536, stream=None, max_bytes=None):
    """Where `pattern` occurs in the file a file set held in device memory decodes to (decompress_files' file arguments and
    decode_rle) -> Found(count, positions, size).  With out = decompress_files(the same arguments) the answer is
    find(out, pattern, max_hits=max_hits), size = out.numel(); raises what that call raises — every block is decoded, so a
    fault is reported whichever group it lies in.  Together with build_index / read_ranges this is the complete "locate, then
    fetch" pair: the positions found here are the ranges read there, and the decoded file never exists for either.
    Neither the decoded file nor a tensor of its size ever exists: verify_files' chain (_ParsedSet.walk, groups that fit
    max_bytes, default a quarter of the free device memory) with find_dev where compare_dev is.
    A group's blocks are one chain (FIND_NEXT), each reported at its offset in the decoded file.  Occurrences over a GROUP
    seam: behind a group's find_dev the last len(pattern) - 1 bytes of the stream so far are copied to a carry (stream
    ordered, before the buffer is used again); in front of the next group's find_dev a seam tensor of that carry and the
    group's first len(pattern) - 1 bytes is searched as two regions, {FIND_NEXT} and {FIND_CONTEXT}.  All calls append into
    one array and one total on the device, so the positions come out ascending without a sort and without a
    synchronisation of their own; behind the last synchronisation the total is read, then the positions kept.  A group
    searched a second time, because a block of it was decoded again, starts from the total (saved on the device) and the
    carry in front of it.  No pack_payloads(RAW) runs; the synchronisations are verify_files'."""
    import torch
    what = "find_files"
    pat, max_hits = _find_args(pattern, max_hits, what)
    m = len(pat)
    with _ParsedSet(what, shaf, cod, rle, freq, stream, max_bytes, decode_rle) as s:
        if s.fb == 0:
            return Found(0, np.empty(0, dtype=np.int64), 0)
        bt, st, dev = s.bt, s.st, s.dev
        res = torch.empty(1 + max_hits, dtype=torch.int64, device=dev)           # the total, then the positions
        d_total, d_hits = res[:1], res[1:] if max_hits else None
        d_total.zero_()
        d_save = torch.zeros(1, dtype=torch.int64, device=dev)
        d_count = torch.zeros(s.fb, dtype=torch.int64, device=dev)
        d_count2 = torch.zeros(2, dtype=torch.int64, device=dev)
        carry = [torch.empty(m, dtype=torch.uint8, device=dev) for _ in range(2)]
        d_seam = torch.empty(2 * m + 16, dtype=torch.uint8, device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))                           # the zeroing above, in front of the stream's work
        s.plan()
        starts = s.starts
        # per group: the carry's and the head's lengths, on the device (from the host's sizes)
        t = [[min(m - 1, starts[a]), min(m - 1, starts[z] - starts[a])] for a, z in s.groups]
        d_seam_n = {a: d for (a, _), d in zip(s.groups, torch.tensor(t, dtype=torch.int64).reshape(-1, 2).to(dev))}

        def search(a, d_a, a_off, a_n, d_a_n, cin):
            """enqueue, for the group of blocks from a on: the seam's search, the group's own, the copy of the new carry
            -> the carry behind the group (which of the two buffers, its length)"""
            ci, cl = cin
            nb, total = len(a_n), sum(a_n)
            if m > 1 and cl and total:
                d_seam[:cl].copy_(carry[ci][:cl])
                hl = 0
                for o, n in zip(a_off, a_n):                                 # the head may span several short blocks
                    take = min(n, m - 1 - hl)
                    if take:
                        d_seam[cl + hl:cl + hl + take].copy_(d_a[o:o + take])
                        hl += take
                    if hl == m - 1:
                        break
                bt.find_dev(st, d_seam, [0, cl], [cl, hl], d_seam_n[a], [FIND_NEXT, FIND_CONTEXT],
                            [starts[a] - cl, starts[a]], pat, max_hits, d_hits, d_count2, d_total)
            bt.find_dev(st, d_a, a_off, a_n, d_a_n, [FIND_NEXT] * (nb - 1) + [0], starts[a:a + nb], pat, max_hits, d_hits,
                        d_count[a:a + nb], d_total)
            if m == 1:
                return cin
            tail, have = [], 0
            for o, n in zip(reversed(a_off), reversed(a_n)):
                take = min(n, m - 1 - have)
                if take:
                    tail.append((o + n - take, take))
                    have += take
                if have == m - 1:
                    break
            old = min(cl, m - 1 - have)                                      # a group shorter than the carry keeps some of it
            nxt = carry[1 - ci]
            if old:
                nxt[:old].copy_(carry[ci][cl - old:cl])
            for o, t in reversed(tail):
                nxt[old:old + t].copy_(d_a[o:o + t])
                old += t
            return 1 - ci, old

        cin, cur = {}, (0, 0)                                                    # the carry in front of each group searched; the last one

        def reader(a, z, d_a, a_off, a_n, d_a_n):
            nonlocal cur
            with torch.cuda.stream(st):
                if a in cin:                                                     # decoded again: searched again, from the total
                    d_total.copy_(d_save)                                        # and the carry in front of the group
                else:
                    d_save.copy_(d_total)
                    cin[a] = cur
                cur = search(a, d_a, a_off, a_n, d_a_n, cin[a])

        s.walk(reader)
        total = int(res[:1].cpu()[0])
        kept = min(total, max_hits)
        return Found(total, res[1:1 + kept].cpu().numpy().copy() if kept else np.empty(0, dtype=np.int64), starts[-1])


# ------------------------------------------------------------------ seek index
SEEK_SF, SEEK_RLE, SEEK_UNINDEXED = 1, 2, 1
SeekBlock = collections.namedtuple("SeekBlock", "decoded_size n_symbols payload_offset payload_size first_checkpoint indexed")


class SeekIndex:
    """What build_index leaves: `checkpoints`, the device tensor (int64, two words a checkpoint: include/shafa_hip.h, "Seek
    index"); `blocks`, the host-side block table (a SeekBlock per block); `span`; `mode` ("N" or "R" for a .shaf + .cod pair,
    "rle" for .rle + .freq); `decoded_size`; `file_lengths`, of the payload file and the text file it was built from.  For
    the two RLE forms the checkpoints' decoded offsets are also kept on the host (8 bytes a checkpoint): read_ranges finds
    the checkpoints that cover a range there."""

    def __init__(self, checkpoints, blocks, span, mode, file_lengths, offsets=None):
        self.checkpoints, self.blocks, self.span, self.mode = checkpoints, list(blocks), int(span), mode
        self.file_lengths = tuple(int(n) for n in file_lengths)
        self.starts = [0]
        for blk in self.blocks:
            self.starts.append(self.starts[-1] + blk.decoded_size)
        self.decoded_size = self.starts[-1]
        self.offsets = offsets

    @property
    def nbytes(self):
        return self.checkpoints.numel() * 8


def _seek_span(span, what):
    if not isinstance(span, int) or not 256 <= span <= 8192 or span & (span - 1):
        raise ValueError(f"{what}: span is a power of two, 256 .. 8192")


def build_index(shaf=None, cod=None, rle=None, freq=None, span=1024, stream=None, max_bytes=None):
    """A seek index of a file set held in device memory (decoded_sizes' file arguments and mode rules) -> SeekIndex: one
    checkpoint every `span` SF symbols of every block (RLE bytes for .rle + .freq), with which read_ranges decodes byte ranges
    from the few hundred stream bytes that cover them.
    Every block is decoded exactly once, in groups that fit max_bytes (default: a quarter of the free device memory) as in
    verify_files' mode-N path — unpack_payloads -> sf_decode_dev -> seek_index_dev on the decoded regions (.rle + .freq:
    unpack_payloads -> seek_index_dev) — so neither the decoded file nor, for a mode-R pair, the .rle stream ever exists.
    Raises what decompress_files raises for the same files, with its precedence (header, mode, SF faults, RLE faults, parse
    faults behind good blocks): after a successful build the files are known to be good.  A block whose table holds a code
    of more than 32 bits is marked unindexed (SeekBlock.indexed is False); read_ranges serves it through decompress_range."""
    import torch
    what = "build_index"
    _seek_span(span, what)
    with _ParsedSet(what, shaf, cod, rle, freq, stream, max_bytes) as s:
        bt, st, dev, sf = s.bt, s.st, s.dev, s.sf
        mode = s.mode if sf else "rle"
        is_rle = mode != "N"
        flags = (SEEK_SF if sf else 0) | (SEEK_RLE if is_rle else 0)
        lengths = (s.files[0].numel(), s.files[1].numel())
        if s.fb == 0:
            return SeekIndex(torch.zeros(0, dtype=torch.int64, device=dev), [], span, mode, lengths,
                             np.zeros(0, dtype=np.int64) if is_rle else None)
        s.plan(measured=False)                                               # the RLE forms: seek_index_dev measures them itself
        nsym = s.sizes
        nck = [max(1, -(-n // span)) for n in nsym]
        first = [0]
        for c in nck:
            first.append(first[-1] + c)
        d_ckpt = torch.zeros(2 * first[-1], dtype=torch.int64, device=dev)
        d_status = torch.zeros(s.fb, dtype=torch.int32, device=dev)
        d_size = torch.zeros(s.fb, dtype=torch.int64, device=dev)
        tsz = C.sizeof(CodeTable)

        def index(a, z, d_a, a_off, a_cap, d_a_n):
            bt.seek_index_dev(st, d_a, a_off, a_cap, d_a_n, s.d_tab[a * tsz:z * tsz] if sf else None, span, flags,
                              first[a:z], d_ckpt, d_status[a:z], d_size[a:z])
        s.walk(index)
        sizes, status, poff = _u64_host(d_size), d_status.cpu().tolist(), _u64_host(s.d_off)
        blocks = [SeekBlock(sizes[i], nsym[i], poff[i], s.pn[i], first[i], status[i] != SEEK_UNINDEXED) for i in range(s.fb)]
        # int64, as the bounds searchsorted is given: another type would make it convert the slice for every range
        offsets = np.ascontiguousarray(d_ckpt.cpu().numpy()[1::2]) if is_rle else None
        return SeekIndex(d_ckpt, blocks, span, mode, lengths, offsets)


def _seek_items(index, spans):
    """(lo, hi, destination) spans of the decoded file -> read_spans' items over the indexed blocks, and (block, lo, hi,
    destination) for the pieces that lie in unindexed blocks"""
    import bisect
    items, other = [], []
    starts, span = index.starts, index.span
    for lo, hi, dst in spans:
        b = bisect.bisect_right(starts, lo) - 1
        while b < len(index.blocks) and starts[b] < hi:
            blk, s0 = index.blocks[b], starts[b]
            l, h = max(lo, s0) - s0, min(hi, starts[b + 1]) - s0
            if l < h:
                at = dst + (s0 + l - lo)
                if not blk.indexed:
                    other.append((b, l, h, at))
                elif index.offsets is None:
                    items.append((b, l // span, (h - 1) // span, l, h, at))
                else:
                    n = max(1, -(-blk.n_symbols // span))
                    w = index.offsets[blk.first_checkpoint:blk.first_checkpoint + n]
                    items.append((b, int(np.searchsorted(w, l, "right")) - 1, int(np.searchsorted(w, h, "left")) - 1, l, h, at))
            b += 1
    return items, other


def read_ranges(index, ranges, shaf=None, cod=None, rle=None, freq=None, stream=None):
    """The byte ranges `ranges` — a sequence of (offset, length), in any order, overlapping or not — of the decoded file of
    the file set `index` was built from -> (out, offsets): range i is out[offsets[i]:offsets[i + 1]] and equals
    decompress_files(...)[offset:offset + length] (Python slice semantics at the end of the file).  A negative offset or
    length, files of another form or of other lengths than the index's: ValueError, before a device is touched.
    One parse of the .cod's tables (unpack_cod, enqueued), ONE read_spans_dev for all ranges and one synchronisation
    (finish); per range only the spans that cover it are decoded, out of the stream bytes where they lie, and nothing
    proportional to a block is allocated.  Pieces in unindexed blocks go through decompress_range, block by block, and are
    copied into place.  Files that are not the indexed ones give other bytes or ShafaError(SHAFA_FILE_UNRECOGNIZABLE)."""
    import torch
    what = "read_ranges"
    if not isinstance(index, SeekIndex):
        raise ValueError(f"{what}: index is a SeekIndex")
    rs = [(int(o), int(n)) for o, n in ranges]
    if any(o < 0 or n < 0 for o, n in rs):
        raise ValueError(f"{what}: negative offset or length")
    sf, files = _decode_args(shaf, cod, rle, freq, what)
    if sf != (index.mode != "rle") or (files[0].numel(), files[1].numel()) != index.file_lengths:
        raise ValueError(f"{what}: these are not the files the index was built from")
    dev, total = files[0].device, index.decoded_size
    offsets, spans = [0], []
    for o, n in rs:
        lo, hi = min(o, total), min(o + n, total)
        if lo < hi:
            spans.append((lo, hi, offsets[-1]))
        offsets.append(offsets[-1] + hi - lo)
    out = torch.empty(offsets[-1], dtype=torch.uint8, device=dev)
    items, other = _seek_items(index, spans)
    if items:
        st = _stream(dev, stream)
        mb = unpack_max_blocks(files[1].numel(), "cod") if sf else 1
        bt = Batch(max(mb, len(index.blocks), len(items)), 1 << 20)
        try:
            d_tab = None
            if sf:
                d_info = torch.zeros(UNPACK_INFO_WORDS, dtype=torch.int64, device=dev)
                d_nsym = torch.zeros(mb, dtype=torch.int64, device=dev)
                d_tab = torch.empty(mb * C.sizeof(CodeTable), dtype=torch.uint8, device=dev)
                bt.unpack_cod(st, mb, files[1], d_info, d_nsym, d_tab)
            blocks = index.blocks
            bt.read_spans_dev(st, files[0], [k.payload_offset for k in blocks], [k.payload_size for k in blocks],
                              [k.n_symbols for k in blocks], [k.first_checkpoint for k in blocks], d_tab, index.span,
                              (SEEK_SF if sf else 0) | (SEEK_RLE if index.mode != "N" else 0), index.checkpoints, items, out)
            _, errs = bt.finish(st, max(mb, len(items)), raise_on_error=False)
            i, e = _first_error(errs[:len(items)])
            if e:
                raise ShafaError(e, f"{what}: block {items[i][0]}")
        finally:
            bt.close()
    for b, l, h, at in other:
        piece = decompress_range(index.starts[b] + l, h - l, shaf=shaf, cod=cod, rle=rle, freq=freq, stream=stream)
        out[at:at + h - l].copy_(piece)
    return out, offsets


def read_range(index, offset, length, **files):
    """read_ranges for one range -> its bytes"""
    return read_ranges(index, [(offset, length)], **files)[0]


MANY_GROUP_SLOTS = 1 << 18      # decompress_many: parse slots per device batch (error words, workspace and tables grow with them)


def _many_entry(e):
    """an entry of decompress_many -> (sf, [payload file, text file], decode_rle), with decompress_files' checks"""
    import torch
    if not isinstance(e, dict) or not set(e) <= {"shaf", "cod", "rle", "freq", "decode_rle"}:
        raise ValueError("decompress_many: an entry is a dict of shaf + cod or rle + freq, and decode_rle")
    if any(e.get(k) is not None and not isinstance(e[k], torch.Tensor) for k in ("shaf", "cod", "rle", "freq")):
        raise ValueError("decompress_many: files are contiguous uint8 CUDA tensors")
    sf, files = _decode_args(e.get("shaf"), e.get("cod"), e.get("rle"), e.get("freq"), "decompress_many")
    return sf, files, bool(e.get("decode_rle", True))


def decompress_many(entries, stream=None, max_bytes=None):
    """decompress_files for many file sets in one device batch.  entries[i] is a dict of decompress_files' file arguments:
    shaf + cod or rle + freq (contiguous uint8 CUDA tensors of any alignment on one device, e.g. compress_many's values) and
    an optional decode_rle.  Element i of the result equals decompress_files(**entries[i]) byte for byte, or is the ShafaError
    instance (not raised) that call would raise, with the same code; other files are unaffected.  Malformed entries, or no
    entries, raise ValueError before any device work.

    Chain per group of files (at most MANY_GROUP_SLOTS parse slots; its length does not depend on the file count): slots per
    file by unpack_max_blocks -> one base per kind of file (the lowest address, offsets are pointer differences, no file is
    copied) -> unpack_cod_files + unpack_shaf_files, unpack_rle_freq_files -> synchronisation 1 (every record and size) ->
    the framed blocks of all files gathered onto consecutive indices (index_select) -> one unpack_payloads -> one sf_decode_dev
    over the blocks of every .shaf file -> pack_payloads_files(RAW) for files without RLE decoding -> synchronisation 2 ->
    each block that lost sf_decode_dev's single 33..64-bit slot decoded again alone (one synchronisation each, one more to pack
    its file again) -> the size pass over every RLE block (rle_decoded_size_dev) and the synchronisation that reads the sizes
    -> rle_decode_dev into regions of exactly those sizes, in groups bounded by max_bytes alone (default: a quarter of the free
    device memory; the launcher cuts its own grids) that follow each other without a synchronisation, each followed by pack_payloads_files(RAW) into exact
    per-file regions -> one last synchronisation.
    Synchronisations per group: 2 without RLE decoding; with it, 4 with .shaf files and 3 for .rle + .freq only, however
    many RLE groups there are.  Decoded blocks are taken MANY_GROUP_BLOCKS at a time (sf_decode_dev puts
    blocks on the grid's y): a group with more repeats the chain after synchronisation 1.  Per file the error is decompress_files':
    a bad header, the mode rule, a parse fault on block 0, SF errors before the first parse fault, RLE errors there, then the
    parse fault."""
    if not isinstance(entries, (list, tuple)) or not entries:
        raise ValueError("decompress_many: no entries")
    parsed = [_many_entry(e) for e in entries]
    dev = parsed[0][1][0].device
    if any(t.device != dev for _, fs, _ in parsed for t in fs):
        raise ValueError("decompress_many: files on more than one device")
    st = _stream(dev, stream)
    max_bytes = _max_bytes(dev, max_bytes)
    results = [None] * len(parsed)
    slots = {}
    for i, (sf, fs, _) in enumerate(parsed):
        mb = unpack_max_blocks(fs[1].numel(), "cod" if sf else "freq")
        if mb > 0x7FFFFFFF:
            results[i] = ShafaError(LACK_OF_MEMORY, "decompress_many: text too long")
        else:
            slots[i] = mb
    group, acc = [], 0
    for i in slots:
        if group and acc + slots[i] > MANY_GROUP_SLOTS:
            _decompress_group(parsed, group, slots, dev, st, max_bytes, results)
            group, acc = [], 0
        group.append(i)
        acc += slots[i]
    if group:
        _decompress_group(parsed, group, slots, dev, st, max_bytes, results)
    return results


def _base(ts):
    """the lowest address of the non-empty tensors (0: none) and each tensor's offset from it"""
    ps = [t.data_ptr() for t in ts if t.numel()]
    b = min(ps) if ps else 0
    return b, [t.data_ptr() - b if t.numel() else 0 for t in ts]


class _Many:
    """one file of a decompress_many group after the parse: its slots, its blocks to decode and its parse fault"""

    def __init__(self, i, sf, rle_after, slot0, fb, perr):
        self.i, self.sf, self.rle_after, self.slot0, self.fb, self.perr = i, sf, rle_after, slot0, fb, perr


def _decompress_group(parsed, files, slots, dev, st, max_bytes, results):
    import torch
    tsz = C.sizeof(CodeTable)
    sfs = [i for i in files if parsed[i][0]]
    rfs = [i for i in files if not parsed[i][0]]
    order = sfs + rfs                                                   # .shaf files' slots first: the tables cover theirs
    first, pos = {}, 0
    for i in order:
        first[i] = pos
        pos += slots[i]
    ns, nsf = pos, sum(slots[i] for i in sfs)
    pbase, poffs = _base([parsed[i][1][0] for i in order])              # .shaf and .rle files: one base
    pend = max([o + parsed[i][1][0].numel() for o, i in zip(poffs, order)])
    with torch.cuda.stream(st):
        # one host read after the parse: the records, the payload sizes and the symbol counts
        meta = torch.zeros(UNPACK_INFO_WORDS * len(order) + ns + nsf, dtype=torch.int64, device=dev)
        info_d = meta[:UNPACK_INFO_WORDS * len(order)]
        d_n = meta[UNPACK_INFO_WORDS * len(order):UNPACK_INFO_WORDS * len(order) + ns]
        d_nsym = meta[UNPACK_INFO_WORDS * len(order) + ns:]
        d_off = torch.zeros(ns, dtype=torch.int64, device=dev)
        d_tab = torch.empty(max(nsf, 1) * tsz, dtype=torch.uint8, device=dev)
        bt = Batch(ns, 1 << 20)
        try:
            if sfs:
                tb, toffs = _base([parsed[i][1][1] for i in sfs])
                fi, mb = [first[i] for i in sfs], [slots[i] for i in sfs]
                bt.unpack_cod_files(st, fi, mb, tb, toffs, [parsed[i][1][1].numel() for i in sfs], info_d, d_nsym, d_tab)
                bt.unpack_shaf_files(st, fi, mb, pbase, poffs[:len(sfs)], [parsed[i][1][0].numel() for i in sfs],
                                     info_d[INFO_INDEXED:], d_off, d_n)
            if rfs:
                tb, toffs = _base([parsed[i][1][1] for i in rfs])
                bt.unpack_rle_freq_files(st, [first[i] for i in rfs], [slots[i] for i in rfs], tb, toffs,
                                         [parsed[i][1][1].numel() for i in rfs], poffs[len(sfs):],
                                         [parsed[i][1][0].numel() for i in rfs], info_d[UNPACK_INFO_WORDS * len(sfs):],
                                         d_off, d_n)
            _, errs = bt.finish(st, ns, raise_on_error=False)           # synchronisation 1
            m = _u64_host(meta)
            n_h = m[UNPACK_INFO_WORDS * len(order):UNPACK_INFO_WORDS * len(order) + ns]
            nsym_h = m[UNPACK_INFO_WORDS * len(order) + ns:]
            todo = []
            for k, i in enumerate(order):                                # _parse_rules, file by file
                sf, _, decode_rle = parsed[i]
                s0, s1 = first[i], first[i] + slots[i]
                try:
                    mode, fb, perr = _parse_rules("decompress_many", m[UNPACK_INFO_WORDS * k:UNPACK_INFO_WORDS * (k + 1)],
                                                  errs[s0:s1], n_h[s0:s1], nsym_h[s0:s1] if sf else None, sf,
                                                  _accepted_modes(sf, decode_rle))
                except ShafaError as e:
                    results[i] = e
                    continue
                if fb == 0:
                    results[i] = torch.empty(0, dtype=torch.uint8, device=dev)
                    continue
                todo.append(_Many(i, sf, not _no_rle_stage(sf, mode, decode_rle), s0, fb, perr))
            part, acc = [], 0
            for f in todo:
                if part and acc + f.fb > MANY_GROUP_BLOCKS:
                    _decode_many(bt, st, dev, part, pbase, pend, d_off, d_n, d_nsym, d_tab, n_h, nsym_h, max_bytes, results)
                    part, acc = [], 0
                part.append(f)
                acc += f.fb
            if part:
                _decode_many(bt, st, dev, part, pbase, pend, d_off, d_n, d_nsym, d_tab, n_h, nsym_h, max_bytes, results)
        finally:
            bt.close()


def _pack_files(bt, st, dev, fs, c0, cnt, d_src, src_off, src_cap, d_src_n, totals):
    """pack_payloads_files(RAW) of files fs (their blocks: c0[f] .. + cnt[f] - 1 of d_src) into exact regions -> views"""
    import torch
    doff, dtot = _layout(totals)
    buf = torch.empty(dtot + 16, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(len(fs), dtype=torch.int64, device=dev)
    bt.pack_payloads_files(st, c0, cnt, FRAME_RAW, d_src, src_off, src_cap, d_src_n, buf, doff, totals, d_len)
    return [buf[o:o + n] for o, n in zip(doff, totals)]


def _decode_many(bt, st, dev, part, pbase, pend, d_off, d_n, d_nsym, d_tab, n_h, nsym_h, max_bytes, results):
    import torch
    tsz = C.sizeof(CodeTable)
    sfp = [f for f in part if f.sf]
    ordered = sfp + [f for f in part if not f.sf]
    idx = []
    for f in ordered:                                                   # block c of the part: slot idx[c]
        f.c0 = len(idx)
        idx.extend(range(f.slot0, f.slot0 + f.fb))
    nb, nsfb = len(idx), sum(f.fb for f in sfp)
    d_idx = torch.tensor(idx, dtype=torch.int64, device=dev)
    d_pn = d_n.index_select(0, d_idx)
    pn = [n_h[s] for s in idx]
    poff, ptot = _layout(pn)
    d_pay = torch.empty(ptot + 16, dtype=torch.uint8, device=dev)
    bt.unpack_payloads_at(st, pbase, pend, d_off.index_select(0, d_idx), d_pn, d_pay, poff, pn)
    rle_in = []                                                         # (file, buffer, offsets, sizes, device sizes)
    if nsfb:
        sidx = d_idx[:nsfb]
        d_ns = d_nsym.index_select(0, sidx)
        d_tb = d_tab.view(-1, tsz).index_select(0, sidx).reshape(-1)
        nsym = [nsym_h[s] for s in idx[:nsfb]]
        ooff, otot = _layout(nsym)
        d_sfo = torch.empty(otot + 16, dtype=torch.uint8, device=dev)
        bt.sf_decode_dev(st, d_pay, poff[:nsfb], pn[:nsfb], d_pn[:nsfb], d_tb, d_ns, d_sfo, ooff, nsym)
        plain = [f for f in sfp if not f.rle_after and not f.perr]
        ptotal = [sum(nsym[f.c0:f.c0 + f.fb]) for f in plain]
        views = _pack_files(bt, st, dev, plain, [f.c0 for f in plain], [f.fb for f in plain], d_sfo, ooff, nsym, d_ns,
                            ptotal) if plain else []
        _, errs = bt.finish(st, nsfb, raise_on_error=False)             # synchronisation 2
        errs = errs[:nsfb]
        again = set()
        args = (d_pay, poff, pn, d_pn, d_tb, d_ns, d_sfo, ooff, nsym)
        faults = any(errs)                                              # none in the whole part: no file has to look
        for f in sfp:                                                   # the one slot for 33..64-bit codes was taken
            b, e = _sf_decode_again(bt, st, args, errs, f.c0, f.c0 + f.fb, again, 1) if faults else (f.fb, SUCCESS)
            f.err = (b, e) if e else None
        redo = [k for k, f in enumerate(plain) if not f.err and any(g in again for g in range(f.c0, f.c0 + f.fb))]
        if redo:
            fs = [plain[k] for k in redo]
            for k, v in zip(redo, _pack_files(bt, st, dev, fs, [f.c0 for f in fs], [f.fb for f in fs], d_sfo, ooff, nsym,
                                              d_ns, [ptotal[k] for k in redo])):
                views[k] = v
            bt.finish(st, nsfb, raise_on_error=False)
        for f in sfp:
            if f.err:
                results[f.i] = ShafaError(f.err[1], f"decompress_many: block {f.err[0]}")
            elif f.perr and not f.rle_after:
                results[f.i] = ShafaError(f.perr, f"decompress_many: block {f.fb}")
            elif f.rle_after:
                rle_in.append((f, d_sfo, ooff[f.c0:f.c0 + f.fb], nsym[f.c0:f.c0 + f.fb], d_ns[f.c0:f.c0 + f.fb]))
        for f, v in zip(plain, views):
            if not f.err:
                results[f.i] = v
    for f in ordered[len(sfp):]:
        rle_in.append((f, d_pay, poff[f.c0:f.c0 + f.fb], pn[f.c0:f.c0 + f.fb], d_pn[f.c0:f.c0 + f.fb]))
    if rle_in:
        _rle_decode_many(bt, st, dev, rle_in, max_bytes, results)


def _rle_decode_many(bt, st, dev, rle_in, max_bytes, results):
    """The RLE stage of these files: the size pass over all their blocks and its synchronisation (decompress_files' rule:
    a file's first refused block in block order is its error), then rle_decode_dev of the files without a fault into regions
    of exactly the measured sizes, in groups (_rle_groups) that follow each other without a synchronisation, each followed by
    pack_payloads_files(RAW) of the group's part of every file; one last synchronisation.  A file whose blocks span groups is
    joined at the end."""
    import torch
    bufs = {id(b): b for _, b, _, _, _ in rle_in}
    lo = min(bufs.values(), key=lambda t: t.data_ptr())                 # inputs addressed from one base
    in_off, in_n, owner = [], [], []
    for k, (f, buf, off, n, _) in enumerate(rle_in):
        a = buf.data_ptr() - lo.data_ptr()
        in_off += [a + o for o in off]
        in_n += n
        owner += [k] * len(n)
    d_in_n = torch.cat([d for _, _, _, _, d in rle_in])
    nb = len(in_n)
    sizes, errs = _rle_measure(bt, st, lo, in_off, in_n, d_in_n, nb)
    err = [None] * len(rle_in)
    for b in range(nb):
        if errs[b] and err[owner[b]] is None:
            err[owner[b]] = errs[b]
    parts = [[] for _ in rle_in]
    sel = [b for b in range(nb) if err[owner[b]] is None and not rle_in[owner[b]][0].perr]
    if sel:
        if len(sel) < nb:
            in_off, in_n, sizes, owner = ([v[b] for b in sel] for v in (in_off, in_n, sizes, owner))
            d_in_n = d_in_n.index_select(0, torch.tensor(sel, dtype=torch.int64, device=dev))
        groups = _rle_groups(sizes, max_bytes)
        biggest = max(_layout(sizes[a:z])[1] for a, z in groups)
        d_out = torch.empty(biggest + 16, dtype=torch.uint8, device=dev)
        d_out_n = torch.zeros(len(sel), dtype=torch.int64, device=dev)
        for a, z in groups:
            off, _ = _layout(sizes[a:z])
            bt.rle_decode_dev(st, lo, in_off[a:z], in_n[a:z], d_in_n[a:z], d_out, off, sizes[a:z], d_out_n[a:z])
            ks, c0, cnt, tot = [], [], [], []
            for b in range(a, z):
                if not ks or ks[-1] != owner[b]:
                    ks.append(owner[b])
                    c0.append(b - a)
                    cnt.append(0)
                    tot.append(0)
                cnt[-1] += 1
                tot[-1] += sizes[b]
            for k, v in zip(ks, _pack_files(bt, st, dev, ks, c0, cnt, d_out, off, sizes[a:z], d_out_n[a:z], tot)):
                parts[k].append(v)
    _, errs = bt.finish(st, nb, raise_on_error=False)
    _, late = _first_error(errs)                                        # the size pass accepted every block decoded: the device
    for k, (f, _, _, _, _) in enumerate(rle_in):
        if err[k]:
            results[f.i] = ShafaError(err[k], "decompress_many: RLE decoding")
        elif f.perr:
            results[f.i] = ShafaError(f.perr, f"decompress_many: block {f.fb}")
        elif late:
            results[f.i] = ShafaError(late, "decompress_many: RLE decoding")
        else:
            results[f.i] = parts[k][0] if len(parts[k]) == 1 else torch.cat(parts[k])


# ------------------------------------------------------------------ Modules T and C alone, on files in device memory
GRID_BLOCKS = 65535             # hist256_tiles and the encoders put blocks on the grid's y


def _file_tensors(what, **files):
    """a module's file arguments checked, before any device work -> them, flattened"""
    import torch
    out = []
    for name, t in files.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{what}: {name} is a contiguous uint8 CUDA tensor")
        if out and t.device != out[0].device:
            raise ValueError(f"{what}: the files are on one device")
        out.append(t.reshape(-1))
    return out


def _bytes_tensor(b, dev):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)


def build_cod(freq, stream=None):
    """Module T alone: the .cod that `shafa X.freq -m t` (get_shafa_codes, host/modules.c) writes for the .freq / .rle.freq
    held in `freq` (a contiguous uint8 CUDA tensor, any alignment), as a uint8 CUDA tensor holding exactly the file.

    Chain: unpack_freq (unpack_max_blocks(n, "counts") slots) -> one synchronisation that reads the header record and the
    blocks' codes -> sf_build_codes -> pack_cod with the file's own mode and sizes -> finish: two synchronisations.
    Errors raise ShafaError with the host's code; Module T handles the blocks strictly one after another, so the first error
    in block order is the host's answer on files with several faults too: a bad header or a mode other than R / N is
    FILE_UNRECOGNIZABLE (modules.c:713), a block whose frame fails FILE_STREAM_FAILED, a block whose counts fail
    shafa_freq_parse FILE_UNRECOGNIZABLE.  A header count of 0 gives the host's "@<mode>@0@0".
    The one divergence: counts whose sum does not fit 64 bits are OUTSIDE_MODULE (sf_build_codes), where the host's sum
    wraps; a block's own histogram cannot get there."""
    import torch
    what = "build_cod"
    f, = _file_tensors(what, freq=freq)
    dev = f.device
    st = _stream(dev, stream)
    mb = unpack_max_blocks(f.numel(), "counts")
    if mb > 0x7FFFFFFF:
        raise ShafaError(LACK_OF_MEMORY, f"{what}: text too long")
    bt = Batch(mb, 1 << 20)
    try:
        d_info = torch.zeros(UNPACK_INFO_WORDS, dtype=torch.int64, device=dev)
        d_sizes = torch.zeros(mb, dtype=torch.int64, device=dev)
        d_counts = torch.empty(mb * 256, dtype=torch.int64, device=dev)
        bt.unpack_freq(st, mb, f, d_info, d_sizes, d_counts)
        _, errs = bt.finish(st, mb, raise_on_error=False)
        info = _u64_host(d_info)
        mode = chr(info[INFO_MODE])
        if info[INFO_STATUS] or mode not in "RN":
            raise ShafaError(FILE_UNRECOGNIZABLE, f"{what}: header")
        nb = info[INFO_INDEXED]
        if info[INFO_COUNT] == 0:
            return _bytes_tensor(f"@{mode}@0@0".encode(), dev)
        b, e = _first_error(errs[:nb])
        if not e and info[INFO_COUNT] > nb:                                  # cannot happen: the slots cover any count
            e = FILE_STREAM_FAILED
        if e:
            raise ShafaError(e, f"{what}: block {b}")
        d_tab = torch.empty(nb * C.sizeof(CodeTable), dtype=torch.uint8, device=dev)
        bt.sf_build_codes(st, nb, d_counts, d_tab)
        buf = torch.empty(pack_cod_max(nb), dtype=torch.uint8, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        bt.pack_cod(st, nb, mode.encode(), d_sizes, d_tab, buf, buf.numel(), d_len)
        _, errs = bt.finish(st, nb, raise_on_error=False)
        b, e = _first_error(errs)
        if e:
            raise ShafaError(e, f"{what}: block {b}")
        return buf[:int(d_len.item())]
    finally:
        bt.close()


def encode_files(d_in, cod, stream=None):
    """Module C alone: the .shaf that `shafa X -m c` (shafa_compress, host/modules.c) writes for the bytes of `d_in` (the
    original, or its .rle) with the code tables of the .cod held in `cod` (contiguous uint8 CUDA tensors on one device, any
    alignment), as a uint8 CUDA tensor holding exactly the file.  Block b encodes the size_b bytes of d_in behind the sum of
    the earlier sizes; bytes of d_in beyond the sum of the sizes are ignored, as the host ignores them.

    Chain: unpack_cod -> a synchronisation that reads the sizes and the blocks' codes (16 bytes a block) -> the blocks'
    inputs in 16-aligned regions (in place when they are, else gathered by unpack_payloads from the prefix sums) ->
    hist256_tiles -> sf_encoded_size_dev -> a synchronisation that reads the encoded sizes -> sf_encode_dev with the parsed
    device tables into regions of those sizes -> pack_payloads(FRAME_SHAF) -> finish: three synchronisations, and output
    memory of the encoded size (the alternative, the host's bound size * Lmax / 8 + 16 of modules.c:859, saves the second
    one and costs up to 32 bytes of output region per input byte).
    Errors raise ShafaError with the host's code, the first in block order, which is the host's answer on files with a single
    fault (with several, the host's depends on how far it reads ahead): a bad header is FILE_UNRECOGNIZABLE (modules.c:808;
    the mode is not judged); a block whose frame fails, or whose size exceeds the input bytes that remain, is
    FILE_STREAM_FAILED, also over a table error of the same block; a text that fails shafa_cod_parse, or a data symbol
    without a code, is FILE_UNRECOGNIZABLE.  A header count of 0 gives "@0".  More than GRID_BLOCKS blocks in one file are
    LACK_OF_MEMORY (one launch takes the file's blocks)."""
    import torch
    what = "encode_files"
    src, text = _file_tensors(what, d_in=d_in, cod=cod)
    dev = src.device
    st = _stream(dev, stream)
    mb = unpack_max_blocks(text.numel(), "cod")
    if mb > 0x7FFFFFFF:
        raise ShafaError(LACK_OF_MEMORY, f"{what}: text too long")
    bt = Batch(mb, 1 << 20)
    try:
        d_info = torch.zeros(UNPACK_INFO_WORDS, dtype=torch.int64, device=dev)
        d_n = torch.zeros(mb, dtype=torch.int64, device=dev)
        d_tab = torch.empty(mb * C.sizeof(CodeTable), dtype=torch.uint8, device=dev)
        bt.unpack_cod(st, mb, text, d_info, d_n, d_tab)
        _, errs = bt.finish(st, mb, raise_on_error=False)
        info = _u64_host(d_info)
        if info[INFO_STATUS]:
            raise ShafaError(FILE_UNRECOGNIZABLE, f"{what}: header")
        if info[INFO_COUNT] == 0:
            return _bytes_tensor(b"@0", dev)
        nidx = info[INFO_INDEXED]
        sizes = _u64_host(d_n)[:nidx]
        # the host's walk: frame, table, then the input's budget, which overrules the table (c_prepare)
        fb, perr, left = nidx, SUCCESS, src.numel()
        if info[INFO_COUNT] > nidx:                                          # cannot happen: the slots cover any count
            perr = FILE_STREAM_FAILED
        for b in range(nidx):
            e = errs[b]
            if e != FILE_STREAM_FAILED and sizes[b] > left:
                e = FILE_STREAM_FAILED
            if e:
                fb, perr = b, e
                break
            left -= sizes[b]
        if fb > GRID_BLOCKS:
            raise ShafaError(LACK_OF_MEMORY, f"{what}: more than {GRID_BLOCKS} blocks")
        if fb == 0:
            raise ShafaError(perr, f"{what}: block 0")
        sizes = sizes[:fb]
        src, off = _aligned_blocks(bt, st, src, [0] + list(itertools.accumulate(sizes))[:-1], sizes, d_n[:fb])
        d_freq = torch.zeros(fb * 256, dtype=torch.int64, device=dev)
        toff, pos = _layout([tile_hist_bytes(n) for n in sizes])
        d_th = torch.empty(pos + 16, dtype=torch.uint8, device=dev)
        d_esize = torch.zeros(fb, dtype=torch.int64, device=dev)
        bt.hist256_tiles(st, src, off, sizes, d_freq, d_th, toff)
        bt.sf_encoded_size_dev(st, fb, d_freq, d_tab, d_esize)
        _, errs = bt.finish(st, fb, raise_on_error=False)
        b, e = _first_error(errs)
        if e or perr:
            raise ShafaError(e or perr, f"{what}: block {b}")
        ocap = [_al16(n) + 16 for n in _u64_host(d_esize)]
        ooff, pos = _layout(ocap)
        d_enc = torch.empty(pos + 16, dtype=torch.uint8, device=dev)
        d_enc_n = torch.zeros(fb, dtype=torch.int64, device=dev)
        bt.sf_encode_dev(st, src, off, sizes, d_n[:fb], d_tab, d_enc, ooff, ocap, d_enc_n, d_th, toff)
        out = torch.empty(pack_payloads_max(ocap, FRAME_SHAF), dtype=torch.uint8, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        bt.pack_payloads(st, FRAME_SHAF, d_enc, ooff, ocap, d_enc_n, out, out.numel(), d_len)
        _, errs = bt.finish(st, fb, raise_on_error=False)
        b, e = _first_error(errs)
        if e:
            raise ShafaError(e, f"{what}: block {b}")
        return out[:int(d_len.item())]
    finally:
        bt.close()


# ------------------------------------------------------------------ typed tensors, one file set per byte plane
PLANES_TILE = 8192              # SHAFA_PLANES_TILE: the elements of one tile of split_planes_dev / merge_planes_dev
PLANES_ELEM = (1, 2, 4, 8)      # the element sizes they take
PLANES_NO_BASE = (1 << 64) - 1  # SHAFA_PLANES_NO_BASE: the base offset of a block without a base (the _xor_dev entries)
PLANES_LAG_STRIP = 256          # SHAFA_PLANES_LAG_STRIP, _ROWS, _ITEMS: the form merge_planes_lag_dev gives a block
PLANES_LAG_ROWS = 32
PLANES_LAG_ITEMS = 4096
PLANES_GRID_LAGS = 3            # SHAFA_PLANES_GRID_LAGS: the lags a block of split_planes_grid_dev / merge_planes_grid_dev may have
PLANES_HIST_RUN = 8             # SHAFA_PLANES_HIST_RUN: the tiles a workgroup of hist_planes_grid_dev counts between two flushes
RECORDS_MAX_WIDTH = 64          # SHAFA_RECORDS_MAX_WIDTH: split_records_dev / merge_records_dev take records of 1 .. 64 bytes
RECORDS_TILE = 8192             # SHAFA_RECORDS_TILE: the records of one tile of theirs


class CompressedTensor:
    """A tensor compressed by byte plane (compress_tensors), in memory: `dtype` and `shape` of the original, `planes` — one
    entry per byte of the element, plane 0 the least significant: the dict compress_many returns for that plane's bytes, or the
    plane itself (a uint8 CUDA tensor) where coding it would not shrink it — and `nbytes`, the sum of the file lengths and of
    the raw planes' lengths."""
    __slots__ = ("dtype", "shape", "planes", "nbytes")

    def __init__(self, dtype, shape, planes, nbytes):
        self.dtype, self.shape, self.planes, self.nbytes = dtype, tuple(shape), list(planes), int(nbytes)

    def __repr__(self):
        kinds = ["raw" if not isinstance(p, dict) else "+".join(sorted(p)) for p in self.planes]
        return f"CompressedTensor({self.dtype}, {self.shape}, planes={kinds}, nbytes={self.nbytes})"


class CompressedDelta(CompressedTensor):
    """A tensor compressed by byte plane as its XOR with a base tensor (compress_deltas): CompressedTensor's fields, the
    planes being those of (element XOR base element), and `base_crc`, the zlib CRC-32 of the base's bytes, or None where the
    base was not digested.  Only decompress_deltas, given that base again, gives the tensor back."""
    __slots__ = ("base_crc",)

    def __init__(self, dtype, shape, planes, nbytes, base_crc=None):
        CompressedTensor.__init__(self, dtype, shape, planes, nbytes)
        self.base_crc = None if base_crc is None else int(base_crc) & 0xFFFFFFFF

    def __repr__(self):
        crc = "None" if self.base_crc is None else f"{self.base_crc:#010x}"
        return "CompressedDelta" + CompressedTensor.__repr__(self)[len("CompressedTensor"):-1] + f", base_crc={crc})"


class CompressedSequence(CompressedTensor):
    """A tensor compressed by byte plane as the differences of its flattened elements (compress_sequences): CompressedTensor's
    fields, the planes being those of the zigzag-folded difference of every element, as an unsigned integer, to the element in
    front.  Only decompress_sequences gives the tensor back."""
    __slots__ = ()

    def __repr__(self):
        return "CompressedSequence" + CompressedTensor.__repr__(self)[len("CompressedTensor"):]


def plane_files(entry):
    """The file arguments of decompress_files / decompress_many for one compressed plane of a CompressedTensor (compress_many's
    dict: with RLE the .rle.shaf decodes through both stages, without the .shaf is the plane)."""
    if ".rle.shaf" in entry:
        return dict(shaf=entry[".rle.shaf"], cod=entry[".rle.cod"])
    return dict(shaf=entry[".shaf"], cod=entry[".cod"], decode_rle=False)


def _plane_tensors(what, ts):
    """the tensors byte planes are taken of, checked before any device work -> a list"""
    import torch
    if isinstance(ts, torch.Tensor):
        ts = [ts]
    if not isinstance(ts, (list, tuple)):
        raise ValueError(f"{what}: a tensor or a list of tensors")
    for t in ts:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{what}: contiguous CUDA tensors")
        if t.element_size() not in PLANES_ELEM:
            raise ValueError(f"{what}: {t.dtype} has elements of {t.element_size()} bytes, not 1, 2, 4 or 8")
        if t.device != ts[0].device:
            raise ValueError(f"{what}: the tensors are on one device")
    return list(ts)


def _plane_stream(dev, stream):
    """the stream a driver works on, ordered behind the caller's current one (which produced the arguments)"""
    import torch
    st = _stream(dev, stream)
    st.wait_stream(torch.cuda.current_stream(dev))
    return st


# The drivers below serve five variants of one chain.  A tensor is `units` = (count, width): its count of units of `width` bytes,
# an element's 1, 2, 4 or 8 or a record's 1 .. RECORDS_MAX_WIDTH; column j of a unit is a plane.  The variant `kind` names the
# pair of Batch methods, split_<kind>_dev / merge_<kind>_dev: "planes", "planes_xor" (with `bases`), "planes_diff", "planes_lag"
# (`bases` holds the tensors' lags), "planes_grid" (`bases` holds the tensors' tuples of lags) or "records".
def _by_width(units):
    """indices of the non-empty tensors, grouped by unit width -> [(width, [index, ...])]"""
    return [(w, [i for i, (n, x) in enumerate(units) if x == w and n]) for w in sorted({x for n, x in units if n})]


def _elements(ts):
    """the units of tensors taken by element"""
    return [(t.numel(), t.element_size()) for t in ts]


def _base_side(bases, idx):
    """the base arguments of a split_planes_xor_dev / merge_planes_xor_dev launch over the tensors idx: the lowest base address
    and each block's offset from it (PLANES_NO_BASE where bases[i] is None); None where no tensor of idx has a base"""
    have = [bases[i].data_ptr() for i in idx if bases[i] is not None] if bases is not None else []
    if not have:
        return None
    return min(have), [PLANES_NO_BASE if bases[i] is None else bases[i].data_ptr() - min(have) for i in idx]


def _transpose(bt, way, kind, side):
    """bt's `way` ("split" / "merge") method of the variant; a "planes_xor" launch none of whose tensors has a base (side is
    None) is the plain one"""
    return getattr(bt, f"{way}_{'planes' if kind == 'planes_xor' and side is None else kind}_dev")


def _lag_side(kind, lags, idx):
    """the lag argument of a split_planes_lag_dev / merge_planes_lag_dev launch over the tensors idx, behind the width (the _grid
    pair: the tuples of lags): a tuple to be spliced in, empty for every other variant"""
    if kind == "planes_grid":
        return ([tuple(lags[i]) for i in idx],)
    return ([int(lags[i]) for i in idx],) if kind == "planes_lag" else ()


def _split_into(bt, st, dev, ts, units, kind, bases=None):
    """one split launch per distinct width over ts (blocks addressed from the lowest tensor address: nothing is concatenated)
    -> the planes buffer and each tensor's plane offsets in it, all multiples of 16.  "planes_xor" with `bases` (one entry per
    tensor: None or a tensor of the same dtype and numel): a width with a base among its tensors takes split_planes_xor_dev, the
    bases addressed from the lowest base address.  "planes_diff": one block a tensor, so the differences run over the
    flattened tensor.  "planes_lag": the same at the distance bases[i], an int, for tensor i.  "planes_grid": the same along every
    lag of the tuple bases[i] in turn."""
    import torch
    poff, pos = [], 0
    for n, w in units:
        step = _al16(n)
        poff.append([pos + j * step for j in range(w)])
        pos += w * step
    buf = torch.empty(pos + 16, dtype=torch.uint8, device=dev)
    groups = _by_width(units)
    if groups:
        d_n = torch.tensor([units[i][0] for _, idx in groups for i in idx], dtype=torch.int64, device=dev)
    at = 0
    for w, idx in groups:
        base = min(ts[i].data_ptr() for i in idx)
        side = _base_side(bases, idx) if kind == "planes_xor" else None
        _transpose(bt, "split", kind, side)(st, w, *_lag_side(kind, bases, idx), base, [ts[i].data_ptr() - base for i in idx],
                                            *(side or ()),
                                            [units[i][0] for i in idx], d_n[at:at + len(idx)], buf,
                                            [o for i in idx for o in poff[i]])
        at += len(idx)
    return buf, poff


def _merge_into(bt, st, dev, planes, outs, units, kind, bases=None):
    """one merge launch per distinct width: planes[i] (the 1-D uint8 plane tensors of tensor i, each of units[i]'s count of
    bytes) -> outs[i].  A plane that is not 16-aligned is copied first.  `kind` and `bases` as _split_into takes them."""
    import torch
    groups = _by_width(units)
    if not groups:
        return
    planes = [[p if p.data_ptr() % 16 == 0 else p.clone() for p in ps] for ps in planes]
    d_n = torch.tensor([units[i][0] for _, idx in groups for i in idx], dtype=torch.int64, device=dev)
    at = 0
    for w, idx in groups:
        pbase = min(p.data_ptr() for i in idx for p in planes[i])
        obase = min(outs[i].data_ptr() for i in idx)
        side = _base_side(bases, idx) if kind == "planes_xor" else None
        _transpose(bt, "merge", kind, side)(st, w, *_lag_side(kind, bases, idx), pbase,
                                            [p.data_ptr() - pbase for i in idx for p in planes[i]], *(side or ()),
                                            [units[i][0] for i in idx], d_n[at:at + len(idx)], obase,
                                            [outs[i].data_ptr() - obase for i in idx])
        at += len(idx)


def _split_one(kind, t, n, w, stream, bases=None):
    """split_planes' / split_records' / split_strided's work on the checked tensor t of n units of w bytes (bases: _split_into's):
    one launch, one synchronisation"""
    import torch
    dev = t.device
    st = _plane_stream(dev, stream)
    with torch.cuda.stream(st):
        bt = Batch(1, 1 << 20)
        try:
            buf, _ = _split_into(bt, st, dev, [t], [(n, w)], kind, bases)
            bt.finish(st, 1)
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return buf[:w * _al16(n)].view(w, _al16(n))[:, :n]


def split_planes(t, stream=None):
    """The byte planes of a contiguous CUDA tensor with elements of k = 1, 2, 4 or 8 bytes: a uint8 tensor [k, numel], row j
    byte j of every element (row 0 the least significant).  Rows start at multiples of 16 bytes: with a numel that is no
    multiple of 16 the result is a view with padded rows.  One split_planes_dev launch, one synchronisation."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("split_planes: a contiguous CUDA tensor")
    t = _plane_tensors("split_planes", t)[0]
    return _split_one("planes", t, t.numel(), t.element_size(), stream)


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _elem_size(what, dtype):
    import torch
    if not isinstance(dtype, torch.dtype):
        raise ValueError(f"{what}: dtype is a torch.dtype")
    return torch.empty((), dtype=dtype).element_size()


def _shape(what, shape):
    try:
        shape = tuple(int(d) for d in shape)
    except TypeError:
        raise ValueError(f"{what}: shape is a sequence of ints") from None
    if any(d < 0 for d in shape):
        raise ValueError(f"{what}: negative dimension")
    return shape


def _plane_dtype(what, dtype, shape):
    """dtype and shape of a tensor to be put together from planes, checked -> (element size, shape, numel)"""
    k = _elem_size(what, dtype)
    if k not in PLANES_ELEM:
        raise ValueError(f"{what}: {dtype} has elements of {k} bytes, not 1, 2, 4 or 8")
    shape = _shape(what, shape)
    return k, shape, _numel(shape)


def _record_dtype(what, dtype, shape, width):
    """dtype, shape and width of a tensor to be put together from columns, checked -> (width, shape, records)"""
    k = _elem_size(what, dtype)
    shape = _shape(what, shape)
    nbytes = _numel(shape) * k
    if nbytes % records._width(what, width):
        raise ValueError(f"{what}: a width of {width} does not divide the tensor's {nbytes} bytes")
    return width, shape, nbytes // width


def _merge_one(kind, planes, dtype, shape, stream, bases=None):
    """merge_planes' / merge_records' / merge_strided's work on the checked planes [w, n] -> the tensor (bases: _merge_into's): one
    launch, one synchronisation"""
    import torch
    w, n = int(planes.shape[0]), int(planes.shape[1])
    dev = planes.device
    st = _plane_stream(dev, stream)
    with torch.cuda.stream(st):
        out = torch.empty(shape, dtype=dtype, device=dev)
        bt = Batch(1, 1 << 20)
        try:
            _merge_into(bt, st, dev, [[planes[j].contiguous() for j in range(w)]], [out], [(n, w)], kind, bases)
            bt.finish(st, 1)
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return out


def merge_planes(planes, dtype, shape, stream=None):
    """split_planes' inverse for one tensor: `planes` is a uint8 CUDA tensor [k, numel] with unit stride along a row (rows may
    be padded, as split_planes leaves them; rows that do not start at a multiple of 16 bytes are copied first) -> a tensor of
    `dtype` (elements of k bytes) and `shape` (numel elements).  One merge_planes_dev launch, one synchronisation."""
    import torch
    k, shape, n = _plane_dtype("merge_planes", dtype, shape)
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.uint8 or not planes.is_cuda or planes.dim() != 2 \
            or (planes.shape[1] > 1 and planes.stride(1) != 1):
        raise ValueError("merge_planes: planes is a uint8 CUDA tensor [k, numel] with contiguous rows")
    if tuple(planes.shape) != (k, n):
        raise ValueError(f"merge_planes: planes of shape {tuple(planes.shape)} for {k} x {n} bytes")
    return _merge_one("planes", planes, dtype, shape, stream)


def _back_to_back(buf, spans):
    """compress_many's / compressed_sizes' first two arguments for the byte ranges `spans` = [(offset, length)] of buf: the
    buffer and the lengths where the ranges follow each other without a gap, else a list of views (which those concatenate)"""
    if all(spans[i][0] + spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1)):
        return buf[spans[0][0]:spans[-1][0] + spans[-1][1]], [n for _, n in spans]
    return [buf[o:o + n] for o, n in spans], None


def _plane_entries(what, ts, units, kind, bases, block_size, stream):
    """compress_tensors' chain over the checked tensors ts of `units`, and in its other variants compress_deltas' (with `bases`,
    _split_into's), compress_sequences', compress_strided's (`bases` the lags), compress_grids' (`bases` the tuples of lags) and
    compress_records': the split, the sizes, the file sets of the planes that shrink -> per tensor its plane entries, and their
    bytes"""
    import torch
    if isinstance(block_size, bool) or not isinstance(block_size, int) or not 0 <= block_size < 1 << 64:
        raise ValueError(f"{what}: block_size is a size in bytes (shafa_block_count's uint64_t)")
    if not ts:
        return [], []
    dev = ts[0].device
    st = _plane_stream(dev, stream)
    with torch.cuda.stream(st):
        bt = Batch(len(ts), 1 << 20)
        try:
            buf, poff = _split_into(bt, st, dev, ts, units, kind, bases)
            bt.finish(st, len(ts))
        finally:
            bt.close()
        entries = _coded_planes(buf, poff, units, block_size, st)
    torch.cuda.current_stream(dev).wait_stream(st)
    return entries, _entry_bytes(entries)


def _coded_planes(buf, poff, units, block_size, st):
    """_plane_entries' half behind the split's finish, on the stream st (current): the planes of `units` at the offsets `poff`
    of the planes buffer `buf` -> per tensor its plane entries, the file set of every plane that shrinks (compressed_sizes ->
    compress_many) and a view of buf for every other"""
    entries = [[buf[o:o + n] for o in poff[i]] for i, (n, _) in enumerate(units)]
    cand = [(i, j) for i, (n, w) in enumerate(units) if n >= 1024 for j in range(w)]
    if cand:
        spans = [(poff[i][j], units[i][0]) for i, j in cand]
        d_in, sizes = _back_to_back(buf, spans)
        sized = compressed_sizes(d_in, sizes, block_size=block_size, stream=st)
        keep = [c for c, e in zip(cand, sized) if isinstance(e, dict) and sum(e.values()) < units[c[0]][0]]
    else:
        keep = []
    if keep:
        d_in, sizes = _back_to_back(buf, [(poff[i][j], units[i][0]) for i, j in keep])
        for (i, j), e in zip(keep, compress_many(d_in, sizes, block_size=block_size, stream=st)):
            if isinstance(e, ShafaError):
                raise e
            entries[i][j] = e
    return entries


def _entry_bytes(entries):
    """per tensor the bytes of its plane entries: the file lengths and the raw planes' lengths"""
    return [sum(sum(int(f.numel()) for f in p.values()) if isinstance(p, dict) else int(p.numel()) for p in ps)
            for ps in entries]


def compress_tensors(tensors, block_size=8 << 20, stream=None):
    """Compress typed tensors by byte plane.  `tensors` is a tensor or a list of tensors: contiguous CUDA tensors on one
    device, any mix of dtypes with elements of 1, 2, 4 or 8 bytes, any shape, empty ones included.  Returns one
    CompressedTensor per tensor; decompress_tensors gives the tensors back bit for bit.

    An order-0 coder sees every byte of an element through one histogram; taken apart, a float's sign and exponent byte codes
    to a fraction of its size while its mantissa bytes do not shrink at all and are kept as they are.  Chain, its number of
    launches independent of the number of tensors: one split_planes_dev per distinct element size over all tensors of that size
    (blocks addressed from the lowest tensor address: nothing is concatenated) into one planes buffer at 16-aligned offsets ->
    compressed_sizes over all planes of 1 KiB or more in one call -> compress_many over exactly the planes whose file set comes
    out smaller than the plane.  Every other plane — one that does not shrink, one under 1 KiB (FILE_TOO_SMALL), an empty one —
    stays raw, as a view of the planes buffer; no payload is ever written for it.  compressed_sizes and compress_many take
    files back to back: they get the planes buffer itself where the planes they are to look at follow each other without a gap
    (every numel a multiple of 16, none skipped), and otherwise a list of views, which they concatenate — one copy of those
    planes.  `block_size` is theirs (the C host's split of a plane into blocks)."""
    ts = _plane_tensors("compress_tensors", tensors)
    entries, nbytes = _plane_entries("compress_tensors", ts, _elements(ts), "planes", None, block_size, stream)
    return [CompressedTensor(t.dtype, t.shape, ps, nb) for t, ps, nb in zip(ts, entries, nbytes)]


def compress_sequences(tensors, block_size=8 << 20, stream=None):
    """compress_tensors of every tensor's differences along its flattened elements — document offsets, position ids, sorted
    ids and COO / CSR indices, timestamps, sampled signals: data whose low bytes walk through all 256 values while the step
    from one element to the next is small.  `tensors` and `block_size` as compress_tensors takes them, and its argument
    ValueErrors; returns one CompressedSequence per tensor, which decompress_sequences gives back bit for bit, whatever the
    dtype and the values: the elements are taken as unsigned integers of their width, the differences wrap, and their zigzag
    fold (small differences of either sign become small values) is what the planes hold.

    Chain: compress_tensors', with one split_planes_diff_dev per element size in place of the plain split — one block a
    tensor, so a tensor's first element is kept as it is and no difference crosses from one tensor into the next; no temporary
    of the differences exists -> compressed_sizes -> compress_many, as there.  Whether the differences code smaller than the
    elements is the caller's to know: nothing is tried both ways."""
    ts = _plane_tensors("compress_sequences", tensors)
    entries, nbytes = _plane_entries("compress_sequences", ts, _elements(ts), "planes_diff", None, block_size, stream)
    return [CompressedSequence(t.dtype, t.shape, ps, nb) for t, ps, nb in zip(ts, entries, nbytes)]


def _base_tensors(what, bases, metas):
    """the bases of a delta call, checked before any device work: a list as long as metas = [(dtype, numel, device)], each
    entry None or a contiguous CUDA tensor of that dtype and numel on that device (a device of None: any one device)"""
    import torch
    if isinstance(bases, torch.Tensor):
        bases = [bases]
    if not isinstance(bases, (list, tuple)) or len(bases) != len(metas):
        raise ValueError(f"{what}: bases is a list with one entry (a tensor or None) per tensor")
    dev = None
    for i, (b, (dtype, n, d)) in enumerate(zip(bases, metas)):
        if b is None:
            continue
        if not isinstance(b, torch.Tensor):
            raise ValueError(f"{what}: base {i} is None or a contiguous CUDA tensor")
        if b.dtype != dtype or b.numel() != n:
            raise ValueError(f"{what}: base {i} is {b.dtype} x {b.numel()}, its tensor {dtype} x {n}")
        if not b.is_cuda or not b.is_contiguous():
            raise ValueError(f"{what}: base {i} is None or a contiguous CUDA tensor")
        if b.device != (d if d is not None else dev if dev is not None else b.device):
            raise ValueError(f"{what}: the tensors and their bases are on one device")
        dev = b.device
    return list(bases)


def _base_crcs(bases, stream):
    """zlib.crc32 of each base's bytes (None for None), digested where they lie: one crc32 call with `sizes` where the bases
    lie back to back in one storage, else one call per base"""
    import torch
    views = [(i, b.reshape(-1).view(torch.uint8)) for i, b in enumerate(bases) if b is not None]
    out = [None] * len(bases)
    if not views:
        return out
    vs = [v for _, v in views]
    joined = all(a.untyped_storage().data_ptr() == vs[0].untyped_storage().data_ptr() and
                 a.data_ptr() + a.numel() == b.data_ptr() for a, b in zip(vs, vs[1:]))
    if joined:
        total = sum(int(v.numel()) for v in vs)
        whole = torch.empty(0, dtype=torch.uint8, device=vs[0].device).set_(vs[0].untyped_storage(), vs[0].storage_offset(),
                                                                            (total,))
        crcs = crc32(whole, [int(v.numel()) for v in vs], stream=stream)
    else:
        crcs = [crc32(v, stream=stream) for v in vs]
    for (i, _), c in zip(views, crcs):
        out[i] = c
    return out


def compress_deltas(tensors, bases, block_size=8 << 20, check_base=True, stream=None):
    """compress_tensors of every tensor's XOR with a base — the checkpoint before it, the model it was tuned from — without
    the XOR ever being stored.  `tensors` as compress_tensors takes them; `bases` is a list as long, each entry None or a
    contiguous CUDA tensor on the same device with its tensor's dtype and numel, at any address (a slice at an odd storage
    offset too).  Returns a CompressedTensor where the base is None — exactly compress_tensors' — and a CompressedDelta
    elsewhere; decompress_deltas with the same bases gives the tensors back bit for bit.  A mismatch raises ValueError before
    any device work.

    Against such a base most elements are bit-identical and the others keep their sign and exponent byte, so the planes of
    the XOR are long runs of zero, which RLE and the Shannon-Fano coder behind it shrink most.  Chain: compress_tensors', with
    one split_planes_xor_dev per element size in place of the plain split (tensors addressed from the lowest tensor address,
    bases from the lowest base address: nothing is concatenated, no temporary of the XOR exists) -> compressed_sizes ->
    compress_many, as there.  With `check_base` the bases are digested first (crc32, where they lie) and every
    CompressedDelta carries its base's zlib CRC-32 as `base_crc`, which decompress_deltas checks: this adds ONE
    synchronisation where the bases lie back to back in one storage (one crc32 call with `sizes`) and one per base otherwise.
    Without it `base_crc` is None and nothing is added."""
    ts = _plane_tensors("compress_deltas", tensors)
    bs = _base_tensors("compress_deltas", bases, [(t.dtype, t.numel(), t.device) for t in ts])
    if not isinstance(check_base, bool):
        raise ValueError("compress_deltas: check_base is a bool")
    crcs = _base_crcs(bs, stream) if check_base and ts else [None] * len(ts)
    entries, nbytes = _plane_entries("compress_deltas", ts, _elements(ts), "planes_xor", bs, block_size, stream)
    return [CompressedTensor(t.dtype, t.shape, ps, nb) if b is None else CompressedDelta(t.dtype, t.shape, ps, nb, c)
            for t, b, ps, nb, c in zip(ts, bs, entries, nbytes, crcs)]


def _merge_items(what, items, kind, bases, check_base, stream, merge_into=None):
    """decompress_tensors' checks and chain over the list `items`, and in its other variants decompress_deltas' (with `bases`,
    one entry per item), decompress_sequences', decompress_strided's (`bases` the items' lags), decompress_grids' (`bases` the
    items' tuples of lags) and decompress_records' (whose messages say "column" for a plane).  `merge_into`: a stand-in for
    _merge_into with its arguments (decompress_fields', whose items take one of two merges)"""
    import torch
    noun, length = ("column", "record count") if kind == "records" else ("plane", "tensor's numel")
    lags = bases if kind in ("planes_lag", "planes_grid") else None          # those variants' `bases` are lags, one entry per item
    if kind != "planes_xor":
        bases = None                                 # only this one has base tensors to check
    if bases is not None:
        for i, (it, b) in enumerate(zip(items, bases)):
            if isinstance(it, CompressedDelta) and b is None:
                raise ValueError(f"{what}: item {i} is a CompressedDelta and needs its base")
            if not isinstance(it, CompressedDelta) and b is not None:
                raise ValueError(f"{what}: item {i} is a plain CompressedTensor and takes no base")
        bases = _base_tensors(what, bases, [(it.dtype, _plane_dtype(what, it.dtype, it.shape)[2], None) for it in items])
    metas, dev = [], None
    for it in items:
        if kind == "records":
            k, shape, n = _record_dtype(what, it.dtype, it.shape, it.width)
            count = f"records of {k} bytes have {k} columns"
        else:
            k, shape, n = _plane_dtype(what, it.dtype, it.shape)
            count = f"{it.dtype} has {k} planes"
        if not isinstance(it.planes, (list, tuple)) or len(it.planes) != k:
            raise ValueError(f"{what}: {count}")
        for p in it.planes:
            if isinstance(p, ShafaError):
                continue
            if isinstance(p, dict):
                fs = [f for f in p.values() if isinstance(f, torch.Tensor)]
                if not ({".shaf", ".cod"} <= set(p) or {".rle.shaf", ".rle.cod"} <= set(p)) or len(fs) != len(p):
                    raise ValueError(f"{what}: a compressed {noun} is compress_many's dict of files")
            elif isinstance(p, torch.Tensor) and p.dtype == torch.uint8 and p.dim() == 1 and p.is_contiguous():
                fs = [p]
            else:
                raise ValueError(f"{what}: a {noun} is a dict of files or a contiguous 1-D uint8 tensor")
            for f in fs:
                if not f.is_cuda:
                    raise ValueError(f"{what}: {noun}s are CUDA tensors")
                if dev is not None and f.device != dev:
                    raise ValueError(f"{what}: the {noun}s are on one device")
                dev = f.device
        metas.append((shape, n, k))
    for it in items:
        for p in it.planes:
            if isinstance(p, ShafaError):
                raise p
    if not items:
        return []
    if bases is not None:
        if any(b is not None and b.device != dev for b in bases):
            raise ValueError(f"{what}: the planes and the bases are on one device")
        if check_base:
            want = [it.base_crc if isinstance(it, CompressedDelta) else None for it in items]
            have = _base_crcs([b if w is not None else None for b, w in zip(bases, want)], stream)
            for i, (w, h) in enumerate(zip(want, have)):
                if w != h:
                    raise ShafaError(FILE_UNRECOGNIZABLE, f"{what}: item {i}: the base's CRC-32 is {h:#010x}, the item was "
                                                          f"made against one of {w:#010x}")
    st = _plane_stream(dev, stream)
    with torch.cuda.stream(st):
        coded = [(i, j) for i, it in enumerate(items) for j, p in enumerate(it.planes) if isinstance(p, dict)]
        planes = [list(it.planes) for it in items]
        if coded:
            for (i, j), r in zip(coded, decompress_many([plane_files(items[i].planes[j]) for i, j in coded], stream=st)):
                if isinstance(r, ShafaError):
                    raise r
                planes[i][j] = r
        for (_, n, _), ps in zip(metas, planes):
            if any(int(p.numel()) != n for p in ps):
                raise ShafaError(FILE_UNRECOGNIZABLE, f"{what}: a {noun}'s length is not the {length}")
        outs = [torch.empty(shape, dtype=it.dtype, device=dev) for it, (shape, _, _) in zip(items, metas)]
        bt = Batch(len(items), 1 << 20)
        try:
            (merge_into or _merge_into)(bt, st, dev, planes, outs, [(n, k) for _, n, k in metas], kind,
                                        lags if lags is not None else bases)
            bt.finish(st, len(items))
        finally:
            bt.close()
    torch.cuda.current_stream(dev).wait_stream(st)
    return outs


def decompress_tensors(items, stream=None):
    """compress_tensors' inverse: `items` is a CompressedTensor or a list of them (their planes on one device) -> the list of
    tensors, each equal to the original bit for bit (NaN payloads, signed zeros, denormals: torch.equal on the bytes).

    Chain: decompress_many over all compressed planes of all items in one call -> one merge_planes_dev per element size,
    straight into the freshly allocated result tensors (a plane tensor that is not 16-aligned is copied first; fresh torch
    allocations are aligned).  A plane entry that is a ShafaError instance, or whose file set fails to decode, raises that
    ShafaError; a decoded or raw plane whose length is not the tensor's numel raises ShafaError(FILE_UNRECOGNIZABLE).  Malformed
    items raise ValueError before any device work."""
    if isinstance(items, CompressedTensor):
        items = [items]
    if not isinstance(items, (list, tuple)) or any(not isinstance(it, CompressedTensor) for it in items):
        raise ValueError("decompress_tensors: a CompressedTensor or a list of them")
    if any(isinstance(it, CompressedDelta) for it in items):
        raise ValueError("decompress_tensors: a CompressedDelta needs its base: decompress_deltas")
    if any(isinstance(it, CompressedSequence) for it in items):
        raise ValueError("decompress_tensors: a CompressedSequence holds differences: decompress_sequences")
    return _merge_items("decompress_tensors", items, "planes", None, False, stream)


def decompress_deltas(items, bases, check_base=True, stream=None):
    """compress_deltas' inverse: `items` is its result (CompressedDelta and CompressedTensor items in any mix, or a single
    one), `bases` the list of their bases — the tensor the item was made against for a CompressedDelta, None for a plain
    CompressedTensor -> the list of tensors, each equal to the original bit for bit.

    Chain: decompress_tensors', with one merge_planes_xor_dev per element size in place of the plain merge: decompress_many
    over all coded planes -> the merge straight into fresh tensors, the bases read where they lie (any alignment; they never
    overlap the fresh results).  Before any device work, each a ValueError: a CompressedDelta whose base is None, a base of
    another dtype or numel, a plain CompressedTensor with a base.  With `check_base` the base of every CompressedDelta that
    carries a `base_crc` is digested first (compress_deltas' rule: one synchronisation more where the bases lie back to back,
    else one per base), and one that digests to another value raises ShafaError(FILE_UNRECOGNIZABLE) naming the item's index,
    before anything is decoded or merged: the XOR with a wrong base is a wrong tensor, not an error any later stage could
    see.  decompress_tensors' errors otherwise."""
    if isinstance(items, CompressedTensor):
        items = [items]
    if not isinstance(items, (list, tuple)) or any(not isinstance(it, CompressedTensor) for it in items):
        raise ValueError("decompress_deltas: a CompressedDelta / CompressedTensor or a list of them")
    if any(isinstance(it, CompressedSequence) for it in items):
        raise ValueError("decompress_deltas: a CompressedSequence holds differences: decompress_sequences")
    if not isinstance(check_base, bool):
        raise ValueError("decompress_deltas: check_base is a bool")
    import torch
    if bases is None or isinstance(bases, torch.Tensor):
        bases = [bases]
    if not isinstance(bases, (list, tuple)) or len(bases) != len(items):
        raise ValueError("decompress_deltas: bases is a list with one entry (a tensor or None) per item")
    return _merge_items("decompress_deltas", items, "planes_xor", list(bases), check_base, stream)


def decompress_sequences(items, stream=None):
    """compress_sequences' inverse: `items` is a CompressedSequence or a list of them (their planes on one device) -> the list
    of tensors, each equal to the original bit for bit.

    Chain: decompress_tensors', with one merge_planes_diff_dev per element size in place of the plain merge: decompress_many
    over all coded planes -> the prefix sums of the unfolded differences straight into fresh tensors.  An item that is not a
    CompressedSequence — a plain CompressedTensor or a CompressedDelta, whose planes hold no differences — is refused with a
    ValueError before any device work.  decompress_tensors' errors otherwise."""
    if isinstance(items, CompressedTensor):
        items = [items]
    if not isinstance(items, (list, tuple)) or any(not isinstance(it, CompressedSequence) for it in items):
        raise ValueError("decompress_sequences: a CompressedSequence or a list of them (compress_sequences' items)")
    return _merge_items("decompress_sequences", items, "planes_diff", None, False, stream)


# ------------------------------------------------------------------ fixed-width records, one file set per byte column
from . import records  # noqa: E402  (_record_dtype asks it for a width's check)
from .records import (CompressedRecords, compress_records, decompress_records, merge_records, records_pass,  # noqa: E402,F401
                      split_records)


# ------------------------------------------------------------------ differences along an axis, one file set per byte plane
from . import strided  # noqa: E402
from .strided import (CompressedStrided, compress_strided, decompress_strided, merge_strided, split_strided)  # noqa: E402,F401


# ------------------------------------------------------------------ differences along up to three axes, one file set per byte plane
from . import grids  # noqa: E402
from .grids import (CompressedGrid, choose_lags, compress_grids, decompress_grids, grid_histograms, grid_sizes,  # noqa: E402,F401
                    merge_grid, split_grid)


# ------------------------------------------------------------------ error-bounded float fields: quantised Lorenzo differences
from . import fields  # noqa: E402
from .fields import (FIELD_SLACK, CompressedField, choose_field_lags, compress_fields, decompress_fields,  # noqa: E402,F401
                     field_histograms, field_rates, field_sizes, fit_abs_error, quantize_field, restore_field)

# ------------------------------------------------------------------ point-wise relative bounds: mantissas rounded to the kept bits
from . import rounding  # noqa: E402
from .rounding import (MANTISSA_BITS, CompressedRounded, compress_rounded, decompress_rounded, fit_keep_bits,  # noqa: E402,F401
                       restore_rounded, round_field, rounded_histograms, rounded_rates, rounded_sizes)

# ------------------------------------------------------------------ error statistics: what a bound costs
from . import quality  # noqa: E402
from .quality import (ERR_WORDS, ErrorStats, field_curve, field_errors, fit_keep_bits_snr, fit_psnr,  # noqa: E402,F401
                      rounded_curve, rounded_errors, tensor_errors, verify_fields, verify_rounded)
