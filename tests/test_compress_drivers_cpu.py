"""CPU-side checks of the Python file drivers (shafa-cd_amd/__init__.py): every public function keeps its name and call
signature, and the compress drivers' argument errors (_many_files) come before a device is touched (no GPU needed)."""
import inspect
import types

import pytest

# the module's public functions and their signatures, written out: a refactor of the drivers must leave them as they are
SIGNATURES = {
    "lib": "()",
    "init_devices": "(devices=None)",
    "set_option": "(name, value)",
    "hist256": "(data)",
    "rle_encode": "(data, want_freq=False)",
    "sf_encode": "(data, table, cap=None, raw_rc=False)",
    "sf_decode": "(data, table, n_symbols, raw_rc=False)",
    "rle_decode": "(data, cap=None, raw_rc=False)",
    "pack_payloads_max": "(src_cap, framing)",
    "pack_cod_max": "(nblocks)",
    "pack_freq_max": "(nblocks)",
    "tile_hist_bytes": "(n)",
    "gen_bytes": "(stream, seed, first_index, d_out, n, d_map=None)",
    "zipf_table": "(s=1.2, nsym=256)",
    "host": "()",
    "sf_build_codes": "(freq)",
    "sf_build_codes_batch": "(freq)",
    "freq_format": "(freq)",
    "freq_parse": "(text)",
    "cod_format": "(table)",
    "cod_parse": "(text)",
    "compress_files": "(d_in, block_size, force_rle=False, force_freq=False, stream=None)",
    "compress_many": "(d_in, sizes=None, block_size=65536, force_rle=False, force_freq=False, stream=None)",
    "rle_encoded_sizes": "(d_in, sizes=None, block_size=65536, stream=None)",
    "shaf_file_bytes": "(block_sizes)",
    "compressed_sizes": "(d_in, sizes=None, block_size=65536, force_rle=False, force_freq=False, stream=None)",
    "unpack_max_blocks": "(text_n, kind)",
    "decompress_files": "(shaf=None, cod=None, rle=None, freq=None, decode_rle=True, stream=None, max_bytes=None)",
    "decoded_sizes": "(shaf=None, cod=None, rle=None, freq=None, stream=None)",
    "decompress_range": "(offset, length, shaf=None, cod=None, rle=None, freq=None, stream=None, max_bytes=None)",
    "verify_files": "(d_in, shaf=None, cod=None, rle=None, freq=None, decode_rle=True, stream=None, max_bytes=None)",
    "crc32_combine": "(crc1, crc2, len2)",
    "crc32": "(d_in, sizes=None, stream=None, _piece=None)",
    "checksum_files": "(shaf=None, cod=None, rle=None, freq=None, decode_rle=True, stream=None, max_bytes=None)",
    "find": "(d_in, pattern, sizes=None, max_hits=65536, stream=None, _piece=None)",
    "find_files": "(pattern, shaf=None, cod=None, rle=None, freq=None, decode_rle=True, max_hits=65536, stream=None, "
                  "max_bytes=None)",
    "build_index": "(shaf=None, cod=None, rle=None, freq=None, span=1024, stream=None, max_bytes=None)",
    "read_ranges": "(index, ranges, shaf=None, cod=None, rle=None, freq=None, stream=None)",
    "read_range": "(index, offset, length, **files)",
    "decompress_many": "(entries, stream=None, max_bytes=None)",
    "build_cod": "(freq, stream=None)",
    "encode_files": "(d_in, cod, stream=None)",
    "plane_files": "(entry)",
    "split_planes": "(t, stream=None)",
    "merge_planes": "(planes, dtype, shape, stream=None)",
    "compress_tensors": "(tensors, block_size=8388608, stream=None)",
    "compress_sequences": "(tensors, block_size=8388608, stream=None)",
    "compress_deltas": "(tensors, bases, block_size=8388608, check_base=True, stream=None)",
    "decompress_tensors": "(items, stream=None)",
    "decompress_deltas": "(items, bases, check_base=True, stream=None)",
    "decompress_sequences": "(items, stream=None)",
}
CLASSES = ["CodeTable", "PipeResult", "PipeBlock", "ShafaError", "Batch", "Pipe", "Verify", "Checksum", "Found", "SeekBlock",
           "SeekIndex", "CompressedTensor", "CompressedDelta", "CompressedSequence"]


def test_public_names_and_signatures_are_unchanged(shafa):
    funcs = {k: str(inspect.signature(v)) for k, v in vars(shafa).items()
             if not k.startswith("_") and isinstance(v, types.FunctionType) and v.__module__ == shafa.__name__}
    assert sorted(funcs) == sorted(SIGNATURES), sorted(set(funcs) ^ set(SIGNATURES))
    bad = {k: (funcs[k], SIGNATURES[k]) for k in funcs if funcs[k] != SIGNATURES[k]}
    assert not bad, bad
    classes = [k for k, v in vars(shafa).items()
               if not k.startswith("_") and isinstance(v, type) and v.__module__ == shafa.__name__]
    assert sorted(classes) == sorted(CLASSES), sorted(set(classes) ^ set(CLASSES))


MANY = ("compress_many", "rle_encoded_sizes", "compressed_sizes")


def test_compress_drivers_refuse_bad_arguments_before_a_device(shafa, monkeypatch):
    import torch
    # any device work would need a stream or a batch: both refuse to be made here
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: pytest.fail("a stream was made"))
    monkeypatch.setattr(shafa, "Batch", lambda *a, **k: pytest.fail("a batch was made"))
    cpu = torch.zeros(4096, dtype=torch.uint8)
    meta = torch.zeros(4096, dtype=torch.uint8, device="meta")
    for name in MANY:
        fn = getattr(shafa, name)
        # no files
        for d_in, sizes in ((cpu, None), (cpu, []), ([], None), ((), None)):
            with pytest.raises(ValueError, match=f"{name}: no files"):
                fn(d_in, sizes)
        # not a contiguous uint8 CUDA tensor: a CPU tensor, other dtypes, a strided view, things that are no tensor
        for d_in in (cpu, [cpu], [cpu, cpu], meta.to(torch.int8), meta.to(torch.float32), meta[::2], None, b"x" * 4096,
                     cpu.numpy(), 5):
            with pytest.raises(ValueError, match=f"{name}: d_in is a contiguous uint8 CUDA tensor"):
                fn(d_in, [4096])
    # compress_files hands its one file to the same check
    for d_in in (cpu, cpu[:100], meta.to(torch.int16), cpu[::2]):
        with pytest.raises(ValueError, match="compress_files: d_in is a contiguous uint8 CUDA tensor"):
            shafa.compress_files(d_in, 65536)
