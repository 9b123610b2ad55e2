"""CPU-side checks of the audio-to-token surface (no GPU involved): the ragged min-max entry point is declared,
exported and bound with the argument list of at_logmel_ragged_f32, and the Python layers above it exist."""
import ctypes
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def declaration(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_ragged_minmax_entry_point_takes_the_ragged_argument_list():
    from audio_tokens_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "audio_tokens_amd.h").read_text(), flags=re.S)
    args = declaration(header, "at_logmel_ragged_minmax_f32")
    assert args == declaration(header, "at_logmel_ragged_f32")
    assert args == ["at_ctx* ctx", "const float* mono", "const at_frontend_clip* plan_dev", "int64_t n_clips",
                    "const at_frontend_totals* totals", "int sample_rate", "int n_fft", "int hop", "int n_mels",
                    "const float* fb_or_null", "float* out", "int layout", "int fuse_l2norm", "int32_t* bad", "void* stream"]
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "at_logmel_ragged_minmax_f32")
    res, argtypes = _lib.SIGNATURES["at_logmel_ragged_minmax_f32"]
    assert (res, argtypes) == _lib.SIGNATURES["at_logmel_ragged_f32"] and len(argtypes) == len(args)
    for decl, ct in zip(args, argtypes):   # pointers as void*, int64_t and int as themselves
        want = ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else ctypes.c_int
        assert ct is want, decl
    assert _lib.load().at_logmel_ragged_minmax_f32.argtypes == argtypes


def test_audio_tokenizer_surface_is_importable():
    from audio_tokens_amd import ops
    from audio_tokens_amd.backend import HipBackend
    from audio_tokens_amd.processors import SpecTokenizer
    from audio_tokens_amd.processors.spectrogram_generator import decode_batch
    assert "AudioTokenizer" in ops.__all__
    assert list(inspect.signature(ops.AudioTokenizer.__init__).parameters)[1:] == [
        "centroids", "sample_rate", "n_fft", "hop_length", "n_mels", "normalize", "conv", "fb", "backend"]
    assert list(inspect.signature(ops.AudioTokenizer.encode).parameters) == ["self", "waveforms", "sample_rates"]
    assert list(inspect.signature(ops.AudioTokenizer.encode_files).parameters) == ["self", "paths"]
    assert list(inspect.signature(SpecTokenizer.tokenize_audio).parameters) == ["self", "audio_files", "tokenized_dir"]
    assert inspect.signature(HipBackend.frontend_ragged).parameters["minmax"].default is False
    assert inspect.signature(ops.LogMelSpectrogram.batch).parameters["normalize"].default is False
    assert callable(decode_batch)
