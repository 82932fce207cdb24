"""``--single`` / ``--count-singles``: what the flags cannot apply to is refused with a ValueError that says why and what to do
instead, by both commands, before anything is written or a device opened.  No device."""
import pytest

import bam_util as bu
import interleaved_model as im


def _inputs(tmp_path):
    a, b, s, bam = tmp_path / "il.fq", tmp_path / "other.fq", tmp_path / "single.fq", tmp_path / "a.bam"
    a.write_bytes(im.from_headers([b"@a/1", b"@a/2"]))
    b.write_bytes(im.from_headers([b"@a/1", b"@a/2"]))
    s.write_bytes(im.from_headers([b"@lone"]))
    bam.write_bytes(bu.write([bu.rec("a", 0x41, "ACGT"), bu.rec("a", 0x81, "ACGT")]))
    return str(a), str(b), str(s), str(bam)


def _no_device(monkeypatch):
    """any attempt to open a device fails the test"""
    from vstrains_amd import pe as host

    def boom(*a, **k):
        raise AssertionError("a device was opened")

    monkeypatch.setattr(host, "Context", boom)


def test_unpaired_input(tmp_path):
    from vstrains_amd import pe_inference as pi

    a, b, s, bam = _inputs(tmp_path)
    assert pi.unpaired_input() == [] and pi.unpaired_input((), False, 4, None, pe_text_from="x") == []  # without the flags nothing changes
    assert pi.unpaired_input([s, tmp_path / "other.fq"]) == [s, b]
    assert pi.unpaired_input([s], True, 1, "singles") == [s] and pi.unpaired_input((), True, 1, "singles") == []
    assert pi.unpaired_input([str(tmp_path / "missing.fq")]) == [str(tmp_path / "missing.fq")]  # (the stream's open names it)
    for mode in (None, "strict"):
        with pytest.raises(ValueError, match="--count-singles.*needs --interleaved --interleaved-singles.*--single FILE"):
            pi.unpaired_input((), True, 1, mode)
    with pytest.raises(ValueError, match="is a BAM file.*samtools fastq"):
        pi.unpaired_input([s, bam])
    with pytest.raises(ValueError, match="--single: unpaired reads are counted in one process only.*run without torchrun"):
        pi.unpaired_input([s], False, 2)
    with pytest.raises(ValueError, match="--single and --count-singles: unpaired reads are counted in one process only"):
        pi.unpaired_input([s], True, 8, "singles")
    with pytest.raises(ValueError, match="--pe-text-from reads the counts of an earlier run"):
        pi.unpaired_input([s], False, 1, None, pe_text_from="aln")
    with pytest.raises(ValueError, match="--count-singles counts unpaired reads.*--pe-text-from"):
        pi.unpaired_input((), True, 1, "singles", pe_text_from="aln")


REFUSALS = [
    ("count_singles_alone", lambda a, b, s, bam: (a, b, ["--count-singles"]), "needs --interleaved --interleaved-singles"),
    ("count_singles_strict", lambda a, b, s, bam: (a, a, ["--interleaved", "--count-singles"]), "needs --interleaved --interleaved-singles"),
    ("single_bam", lambda a, b, s, bam: (a, b, ["--single", s, "--single", bam]), "is a BAM file"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0])
def test_both_commands_refuse_before_a_device_is_opened(tmp_path, monkeypatch, case):
    from vstrains_amd import cli, pe_inference as pi

    _, make, why = case
    fwd, rve, flags = make(*_inputs(tmp_path))
    _no_device(monkeypatch)
    monkeypatch.delenv("VS_FASTQ_STREAM", raising=False)
    out = tmp_path / "out"
    with pytest.raises(ValueError, match=why):
        pi.main(["-g", str(tmp_path / "none.gfa"), "-o", str(out), "-f", fwd, "-r", rve, "-k", "21"] + flags)
    with pytest.raises(ValueError, match=why):
        cli.main(["-a", "spades", "-g", str(tmp_path / "none.gfa"), "-p", str(tmp_path / "none.paths"), "-o", str(out), "-fwd", fwd, "-rve", rve] + flags)
    assert not out.exists()  # nothing was written


def test_both_commands_refuse_a_process_group(tmp_path, monkeypatch):
    from vstrains_amd import cli, pe_inference as pi

    a, b, s, _ = _inputs(tmp_path)
    _no_device(monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", "2")  # (torchrun's; the refusal comes before a process group is made)
    with pytest.raises(ValueError, match="one process only"):
        pi.main(["-g", str(tmp_path / "none.gfa"), "-o", str(tmp_path / "out"), "-f", a, "-r", b, "--single", s])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setattr(pi, "_rank_world", lambda: (1, 2))
    with pytest.raises(ValueError, match="one process only"):
        cli.main(["-a", "spades", "-g", str(tmp_path / "none.gfa"), "-p", str(tmp_path / "none.paths"), "-o", str(tmp_path / "out"), "-fwd", a, "-rve", b,
                  "--single", s])
    with pytest.raises(ValueError, match="one process only"):
        pi.count_links(None, str(tmp_path / "none.gfa"), a, b, 21, single=[s])
    assert not (tmp_path / "out").exists()


def test_cli_refuses_the_flags_with_pe_text_from(tmp_path, monkeypatch):
    from vstrains_amd import cli

    a, b, s, _ = _inputs(tmp_path)
    _no_device(monkeypatch)
    base = ["-a", "spades", "-g", str(tmp_path / "none.gfa"), "-p", str(tmp_path / "none.paths"), "-o", str(tmp_path / "out"), "-fwd", a, "-rve", b,
            "--pe-text-from", str(tmp_path / "aln")]
    with pytest.raises(ValueError, match="--single counts unpaired reads, and --pe-text-from reads the counts of an earlier run"):
        cli.main(base + ["--single", s])
    with pytest.raises(ValueError, match="--count-singles counts unpaired reads, and --pe-text-from"):
        cli.main(base + ["--count-singles"])
    assert not (tmp_path / "out").exists()


def test_the_flags_are_off_by_default():
    from vstrains_amd import cli

    args = cli.build_parser().parse_args(["-a", "spades", "-g", "g", "-fwd", "f", "-rve", "r"])
    assert args.single == [] and args.count_singles is False
    args = cli.build_parser().parse_args(["-a", "spades", "-g", "g", "-fwd", "f", "-rve", "r", "--single", "x", "--single", "y"])
    assert args.single == ["x", "y"]
