"""`juliet --batch`: what the command line refuses.  Every refusal ends the process with status 1 and a message before any
BAM is read or any GPU work starts, so these tests need no GPU (the listed BAMs need not even exist)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JULIET = os.path.join(ROOT, "minorseq_amd", "bin", "juliet")


@pytest.fixture(scope="module", autouse=True)
def built():
    """The front end links the library: build both only if they are missing."""
    if not os.path.exists(os.path.join(ROOT, "minorseq_amd", "libjuliet_hip.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "csrc")])
    if not os.path.exists(JULIET):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "minorseq_amd", "host")])


def juliet(cwd, *args):
    return subprocess.run([JULIET, *args], cwd=cwd, capture_output=True, text=True, timeout=60)


def refused(r, *words):
    assert r.returncode == 1, (r.returncode, r.stderr)
    for w in words:
        assert w in r.stderr, (w, r.stderr)


def good_list(d):
    (d / "ok.tsv").write_text("# barcode list\n\na.bam\ta.json\ta.html\nb.bam\tb.json\n")
    return "ok.tsv"


def test_help_mentions_batch():
    r = subprocess.run([JULIET, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--batch" in r.stderr


def test_missing_or_unreadable_list(tmp_path):
    refused(juliet(tmp_path, "--batch", "nope.tsv"), "nope.tsv", "cannot be read")
    (tmp_path / "dir.tsv").mkdir()
    refused(juliet(tmp_path, "--batch", "dir.tsv"), "dir.tsv")
    (tmp_path / "empty.tsv").write_text("# nothing here\n\n")
    refused(juliet(tmp_path, "--batch", "empty.tsv"), "names no sample")


def test_line_with_one_field(tmp_path):
    (tmp_path / "l.tsv").write_text("a.bam\ta.json\n# comment\nb.bam b.json\n")
    refused(juliet(tmp_path, "--batch", "l.tsv"), "line 3", "tabs")


def test_output_of_unknown_kind(tmp_path):
    (tmp_path / "l.tsv").write_text("\na.bam\ta.json\nb.bam\tb.json\tb.txt\n")
    refused(juliet(tmp_path, "--batch", "l.tsv"), "line 3", "b.txt", ".json or .html")


def test_same_output_on_two_lines(tmp_path):
    (tmp_path / "l.tsv").write_text("a.bam\tout.json\nb.bam\t./out.json\n")
    refused(juliet(tmp_path, "--batch", "l.tsv"), "line 2", "line 1")
    (tmp_path / "m.tsv").write_text("a.bam\ta.json\nb.bam\tb.html\tsub/../a.json\n")
    refused(juliet(tmp_path, "--batch", "m.tsv"), "line 2")


def test_positional_arguments_with_batch(tmp_path):
    lst = good_list(tmp_path)
    refused(juliet(tmp_path, "--batch", lst, "in.bam", "out.json"), "--batch")
    refused(juliet(tmp_path, "in.bam", "--batch", lst), "--batch")


@pytest.mark.parametrize("extra, word", [
    (["--windows", "2"], "--windows"),
    (["--devices", "0,1"], "--devices"),
    (["--consensus", "c.fasta"], "--consensus"),
    (["--dump-msa", "m.bin"], "--dump-msa"),
    (["--dump-config", "c.json"], "--dump-config"),
])
def test_options_a_batch_cannot_take(tmp_path, extra, word):
    refused(juliet(tmp_path, *extra, "--batch", good_list(tmp_path)), "--batch", word)
    assert not any(p.suffix in (".json", ".html", ".fasta", ".bin") for p in tmp_path.iterdir())
