"""The device route of the index builder, as far as a machine without a GPU can see it: the entry points exist,
check their arguments, and refuse to run -- they never fall back to the host builder.  (What the route computes:
tests/test_gpu_index_build.py.)"""
import ctypes as C
import glob
import os

import pytest


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


def _entries():
    names = [b"a", b"b"]
    seqs = [b"ACGTACGTTTGACCA", b"GGGNACGT"]
    return (C.c_char_p * 2)(*names), (C.c_char_p * 2)(*seqs)


def test_null_arguments_are_errors_not_crashes(native_lib):
    from mirge_amd import _native
    L = native_lib
    names, seqs = _entries()
    out = C.c_void_p()
    assert L.mrg_index_build_device(0, None, None, 1, C.byref(out)) == _native.MRG_ERR_ARG
    assert b"null" in L.mrg_last_error()
    assert L.mrg_index_build_device(0, names, None, 2, C.byref(out)) == _native.MRG_ERR_ARG
    assert L.mrg_index_build_device(0, None, seqs, 2, C.byref(out)) == _native.MRG_ERR_ARG
    assert L.mrg_index_build_device(0, names, seqs, 2, None) == _native.MRG_ERR_ARG
    assert L.mrg_index_build_fasta_device(0, None, C.byref(out)) == _native.MRG_ERR_ARG
    assert L.mrg_index_build_fasta_device(0, b"/nonexistent.fa", None) == _native.MRG_ERR_ARG
    assert not out.value
    assert L.mrg_index_build_device_rounds() >= 0


def test_capi_refuses_without_gpu(native_lib):
    _no_gpu()
    from mirge_amd import _native
    names, seqs = _entries()
    out = C.c_void_p()
    assert native_lib.mrg_index_build_device(0, names, seqs, 2, C.byref(out)) == _native.MRG_ERR_NO_DEVICE
    assert b"no host fallback" in native_lib.mrg_last_error()
    assert native_lib.mrg_index_build_fasta_device(0, b"/nonexistent.fa", C.byref(out)) == _native.MRG_ERR_NO_DEVICE
    assert not out.value


def test_python_build_raises_without_gpu(native_lib, tmp_path):
    _no_gpu()
    from mirge_amd import _native
    from mirge_amd.index import FmIndex
    with pytest.raises(_native.MirgeAmdError) as ei:
        FmIndex.build(["a", "b"], ["ACGTACGTTTGACCA", "GGGNACGT"], device=0)
    assert ei.value.code == _native.MRG_ERR_NO_DEVICE
    fa = tmp_path / "lib.fa"
    fa.write_text(">a\nACGTACGTTTGACCA\n")
    with pytest.raises(_native.MirgeAmdError) as ei:
        FmIndex.from_fasta(str(fa), device=0)
    assert ei.value.code == _native.MRG_ERR_NO_DEVICE
    with pytest.raises(_native.MirgeAmdError) as ei:
        FmIndex.open_prefix(str(tmp_path / "lib"), device=0)
    assert ei.value.code == _native.MRG_ERR_NO_DEVICE
    # the host builder is untouched by the new parameter
    assert FmIndex.build(["a"], ["ACGTACGTTTGACCA"], device=None).info.n_bases == 15
    assert FmIndex.open_prefix(str(tmp_path / "lib")).info.n_bases == 15


def test_build_index_cli_fails_without_gpu(native_lib, tmp_path, capsys):
    _no_gpu()
    from mirge_amd import build_index
    fa = tmp_path / "lib.fa"
    fa.write_text(">a\nACGTACGTTTGACCA\n>b\nGGGNACGT\n")
    assert build_index.main([str(fa), "--device", "0"]) == 1
    assert build_index.main([str(fa), "--device", "0", "--max-bases", "20"]) == 1
    assert glob.glob(str(tmp_path / "*.mrgfm")) == []
    assert "no HIP device" in capsys.readouterr().err
    # without the option: the host builder, as before
    assert build_index.main([str(fa)]) == 0
    assert os.path.isfile(str(tmp_path / "lib.mrgfm"))


def test_bowtie_build_does_not_fall_back_without_gpu(native_lib, tmp_path, monkeypatch):
    _no_gpu()
    from mirge_amd import bowtie
    fa = tmp_path / "clusters.fa"
    fa.write_text(">a\nACGTACGTTTGACCA\n")
    monkeypatch.setenv("MIRGE_AMD_BUILD_GPU", "0")
    assert bowtie.build_main([str(fa), str(tmp_path / "dev")]) == 1
    assert not os.path.exists(str(tmp_path / "dev.mrgfm"))
    monkeypatch.delenv("MIRGE_AMD_BUILD_GPU")
    assert bowtie.build_main([str(fa), str(tmp_path / "host")]) == 0
    assert os.path.isfile(str(tmp_path / "host.mrgfm"))
