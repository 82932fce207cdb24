"""Host-side parts of the streamed FASTQ ingest that need no device: which inputs take it, and its C ABI."""
import os
import re

from conftest import ROOT


def test_streamed_path_for_inputs_that_are_not_regular_files(tmp_path, monkeypatch):
    from vstrains_amd import pe_inference

    monkeypatch.delenv("VS_FASTQ_STREAM", raising=False)
    (tmp_path / "f.fq").write_text("")
    (tmp_path / "r.fq.gz").write_bytes(b"")
    os.mkfifo(tmp_path / "pipe")
    f, r, pipe = str(tmp_path / "f.fq"), str(tmp_path / "r.fq.gz"), str(tmp_path / "pipe")
    assert not pe_inference.use_stream(f, r)  # regular files (gzip or not) keep the mapped path
    assert pe_inference.use_stream(pipe, r)
    assert pe_inference.use_stream(f, pipe)
    assert not pe_inference.use_stream(f, str(tmp_path / "missing.fq"))  # (the mapped open names the missing file)
    monkeypatch.setenv("VS_FASTQ_STREAM", "1")
    assert pe_inference.use_stream(f, r)
    monkeypatch.setenv("VS_FASTQ_STREAM", "0")
    assert not pe_inference.use_stream(f, r)


def test_stream_entries_declared_and_bound():
    from vstrains_amd import _native

    header = open(os.path.join(ROOT, "include", "vstrains_hip.h")).read()
    for name in ("vs_fastq_stream_open", "vs_fastq_stream_next", "vs_fastq_stream_info", "vs_fastq_stream_close", "vs_fastq_scan_text"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.SYMBOLS
        assert hasattr(_native.lib(), name)
