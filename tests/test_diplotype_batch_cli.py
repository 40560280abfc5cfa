"""`starphase_hip diplotype-batch` without a device: the manifest (header lines, '-' and empty fields, comma-separated BAMs, the column count),
the row-numbered checks made before the first device call (NOINPUT for a missing file, USAGE for settings a row fails), the help texts, and the
debug folder rule (a manifest column; the handle-wide --output-debug of `diplotype` is refused)."""
import os
import subprocess

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DB = os.path.join(GOLDEN, "variant_dbs", "CACNA1S.json")
VCF = os.path.join(GOLDEN, "vcf", "CACNA1S", "hom.vcf.gz")
HEADER = "#output_calls\tbams\tvcf\tsample_name\tsv_vcf\tpharmcat_tsv\toutput_debug\n"


def run_cli(pkg, *args, timeout=120):
    exe = pkg.database.cli_path()
    assert os.path.exists(exe), "build() makes the starphase_hip executable next to the library"
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def no_device():
    import torch
    return not torch.cuda.is_available()


@pytest.fixture
def fasta(tmp_path):
    p = tmp_path / "ref.fa"
    p.write_text(">chr1\nACGT\n")
    return str(p)


def manifest(tmp_path, rows, header=True):
    p = tmp_path / "samples.tsv"
    p.write_text((HEADER if header else "") + "".join("\t".join(r) + "\n" for r in rows))
    return str(p)


def test_help_lists_the_subcommand_and_its_flags(pkg):
    top = run_cli(pkg, "--help")
    assert top.returncode == 0 and "diplotype-batch" in top.stdout and "  diplotype " in top.stdout
    out = run_cli(pkg, "diplotype-batch", "--help")
    assert out.returncode == 0
    for flag in ("--database", "--reference", "--manifest", "--max-group", "--threads", "--include-set", "--max-sv-length", "--min-consensus-count",
                 "output_calls", "pharmcat_tsv", "output_debug"):
        assert flag in out.stdout, flag
    # `diplotype` itself is unchanged
    assert "--output-calls" in run_cli(pkg, "diplotype", "--help").stdout


def test_command_line_errors(pkg, tmp_path, fasta):
    m = manifest(tmp_path, [[str(tmp_path / "a.json"), "-", VCF, "-", "-", "-", "-"]])
    assert run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta).returncode == 2                          # --manifest missing
    assert run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", m, "--bogus").returncode == 2
    assert run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", m, "--max-group", "many").returncode == 2
    out = run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", str(tmp_path / "none.tsv"))
    assert out.returncode == 66 and "Manifest does not exist" in out.stderr
    # the files of one sample are manifest columns: the single-sample flags are refused by name
    for flag in (["--output-debug", str(tmp_path / "dbg")], ["--vcf", VCF], ["--bam", VCF], ["-o", "x.json"]):
        out = run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", m, *flag)
        assert out.returncode == 64 and flag[0] in out.stderr and "column of the manifest" in out.stderr, (flag, out.stderr)
    assert not (tmp_path / "dbg").exists() and not (tmp_path / "a.json").exists()


def test_manifest_column_count_is_checked_with_its_row(pkg, tmp_path, fasta):
    m = manifest(tmp_path, [[str(tmp_path / "a.json"), "-", VCF, "-", "-", "-", "-"], [str(tmp_path / "b.json"), "-", VCF]])
    out = run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", m)
    assert out.returncode == 64 and "manifest row 2 (line 3)" in out.stderr and "expected 7" in out.stderr and "found 3" in out.stderr, out.stderr
    m = manifest(tmp_path, [["-", "-", VCF, "-", "-", "-", "-"]])
    out = run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", m)
    assert out.returncode == 64 and "row 1" in out.stderr and "output_calls is required" in out.stderr
    out = run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", manifest(tmp_path, []))
    assert out.returncode == 64 and "no samples" in out.stderr


def test_missing_files_are_noinput_with_their_row(pkg, tmp_path, fasta):
    ok = [str(tmp_path / "a.json"), "", VCF, "", "", "", ""]                       # empty fields = none
    for bad, label in (([str(tmp_path / "b.json"), "-", str(tmp_path / "no.vcf"), "-", "-", "-", "-"], "VCF file"),
                       ([str(tmp_path / "b.json"), f"{VCF},{tmp_path / 'no.bam'}", VCF, "-", "-", "-", "-"], "Alignment file"),     # comma-separated BAMs
                       ([str(tmp_path / "b.json"), "-", VCF, "-", str(tmp_path / "no_sv.vcf"), "-", "-"], "SV VCF file")):
        out = run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", manifest(tmp_path, [ok, bad]))
        assert out.returncode == 66 and f"manifest row 2: {label} does not exist" in out.stderr, out.stderr
    assert not (tmp_path / "a.json").exists()


def test_settings_check_runs_per_row(pkg, tmp_path, fasta):
    rows = [[str(tmp_path / "a.json"), "-", VCF, "-", "-", "-", "-"], [str(tmp_path / "b.json"), "-", "-", "-", "-", "-", "-"]]
    out = run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", manifest(tmp_path, rows))
    assert out.returncode == 64 and "manifest row 2: Error while processing CLI settings: Must provide a VCF file and/or aligned BAM file" in out.stderr, out.stderr
    # a rule that only applies to a sample with BAMs fails that row alone
    rows = [[str(tmp_path / "a.json"), "-", VCF, "-", "-", "-", "-"], [str(tmp_path / "b.json"), VCF, "-", "-", "-", "-", "-"]]
    out = run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", manifest(tmp_path, rows), "--expected-maf", "0.7")
    assert out.returncode == 64 and "manifest row 2:" in out.stderr and "--expected-maf must be between 0.01 and 0.5" in out.stderr, out.stderr
    out = run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", manifest(tmp_path, rows[:1]), "--include-set", DB, "--exclude-set", DB)
    assert out.returncode == 64 and "manifest row 1:" in out.stderr and "Only one of --exclude-set and --include-set" in out.stderr


def test_valid_manifest_reaches_the_device(pkg, tmp_path, fasta):
    """headers anywhere, '-' and empty fields, a debug folder column: every check passes and, without a device, the handle cannot be made"""
    if not no_device():
        pytest.skip("GPU present: tests/test_gpu_diplotype_batch.py runs the batch")
    p = tmp_path / "samples.tsv"
    p.write_text(HEADER + "# a comment line\n" + "\t".join([str(tmp_path / "a.json"), "", VCF, "-", "", "-", str(tmp_path / "d1" / "x")]) + "\n\n" +
                 "\t".join([str(tmp_path / "b.json"), "-", VCF, "", "-", str(tmp_path / "b.tsv"), "-"]) + "\n")
    out = run_cli(pkg, "diplotype-batch", "-d", DB, "-r", fasta, "--manifest", str(p), "-t", "2", "--max-group", "1")
    assert out.returncode == 69, out.stderr
    assert (tmp_path / "d1" / "x").is_dir()                                      # create_dir_all of the row's debug folder, as `diplotype` does
    assert not (tmp_path / "a.json").exists() and not (tmp_path / "b.json").exists()
