"""The files-to-files entry (sp_diplotype_settings_*, sp_starphase_*, the `starphase_hip diplotype` command) without a device: the defaults and
checks of DiplotypeSettings (src/cli/diplotype.rs:14-330), the command line's flags and exit codes (src/main.rs), and no fallback without a GPU."""
import os
import subprocess

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DB = os.path.join(GOLDEN, "variant_dbs", "CACNA1S.json")
VCF = os.path.join(GOLDEN, "vcf", "CACNA1S", "hom.vcf.gz")

# the reference's default_values (src/cli/diplotype.rs:14-196)
REFERENCE_DEFAULTS = {"include_set": None, "exclude_set": None, "sample_name": None, "sv_vcf": None, "debug_folder": None,
                      "max_sv_length": 1000000, "disable_cdna_scoring": 0, "hla_require_dna": 0, "max_error_rate": 0.07, "min_cdf_prob": 0.001,
                      "expected_maf": 0.45, "infer_connections": 0, "normalize_d6_only": 0, "min_consensus_fraction": 0.10, "min_consensus_count": 3,
                      "dual_max_ed_delta": 100, "debug_skip_hla": 0, "sequential": 0}


def run_cli(pkg, *args, timeout=120):
    exe = pkg.database.cli_path()
    assert os.path.exists(exe), "build() makes the starphase_hip executable next to the library"
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def test_settings_default_is_the_reference_table(pkg):
    assert pkg.database.settings_default() == REFERENCE_DEFAULTS


@pytest.mark.parametrize("kw, message", [
    (dict(bams=(), vcf=None), "Must provide a VCF file and/or aligned BAM file to perform diplotyping."),
    (dict(vcf="x.vcf", include_set="a", exclude_set="b"), "Only one of --exclude-set and --include-set can be specified."),
    (dict(bams=["x.bam"], max_error_rate=1.5), "--max-error-rate must be between 0.0 and 1.0"),
    (dict(bams=["x.bam"], min_cdf_prob=-0.1), "--min-cdf-prob must be between 0.0 and 1.0"),
    (dict(bams=["x.bam"], expected_maf=0.6), "--expected-maf must be between 0.01 and 0.5"),
    (dict(bams=["x.bam"], expected_maf=0.005), "--expected-maf must be between 0.01 and 0.5"),
    (dict(bams=["x.bam"], min_consensus_fraction=1.01), "--min-consensus-fraction must be between 0.0 and 1.0"),
])
def test_settings_check_messages(pkg, kw, message):
    rc, msg, _s = pkg.database.settings_check(**kw)
    assert rc == 1 and msg == message                             # SP_ERR_INVALID_ARG


def test_settings_check_passes_and_adjusts(pkg):
    # the range checks belong to the BAM settings: a VCF-only run is not held to them (check_diplotype_settings, :265-327)
    rc, msg, _s = pkg.database.settings_check(vcf="x.vcf", expected_maf=0.9)
    assert rc == 0 and msg == ""
    rc, _m, s = pkg.database.settings_check(bams=["x.bam"], disable_cdna_scoring=1)
    assert rc == 0 and s["hla_require_dna"] == 1                 # "Automatically enabling HLA DNA requirement"
    rc, _m, s = pkg.database.settings_check(vcf="x.vcf", disable_cdna_scoring=1)
    assert rc == 0 and s["hla_require_dna"] == 0


def test_cli_help_lists_the_flags(pkg):
    out = run_cli(pkg, "diplotype", "--help")
    assert out.returncode == 0
    for flag in ("--database", "--reference", "--vcf", "--sv-vcf", "--bam", "--output-calls", "--pharmcat-tsv", "--include-set", "--exclude-set",
                 "--output-debug", "--sample-name", "--max-sv-length", "--hla-require-dna", "--max-error-rate", "--min-cdf-prob", "--expected-maf",
                 "--infer-connections", "--normalize-d6-only", "--min-consensus-fraction", "--min-consensus-count", "--dual-max-ed-delta",
                 "--sequential", "[default: 1000000]", "[default: 0.45]"):
        assert flag in out.stdout, flag


def test_cli_usage_errors_come_before_any_device_call(pkg, tmp_path):
    fasta = tmp_path / "ref.fa"
    fasta.write_text(">chr1\nACGT\n")
    base = ["diplotype", "-d", DB, "-r", str(fasta), "-o", str(tmp_path / "out.json")]
    # clap: a missing required flag / an unknown flag / a bad number
    assert run_cli(pkg, "diplotype", "-d", DB).returncode == 2
    assert run_cli(pkg, *base, "--vcf", VCF, "--no-such-flag").returncode == 2
    assert run_cli(pkg, *base, "--vcf", VCF, "--max-sv-length", "many").returncode == 2
    # check_required_filename: NOINPUT
    out = run_cli(pkg, "diplotype", "-d", str(tmp_path / "missing.json"), "-r", str(fasta), "-o", str(tmp_path / "o.json"), "--vcf", VCF)
    assert out.returncode == 66 and "Database JSON does not exist" in out.stderr
    assert run_cli(pkg, *base, "--vcf", str(tmp_path / "missing.vcf")).returncode == 66
    # check_diplotype_settings: USAGE with the reference's message
    for extra, message in ((["--bam", VCF, "--expected-maf", "0.7"], "--expected-maf must be between 0.01 and 0.5"),
                           (["--vcf", VCF, "--include-set", DB, "--exclude-set", DB], "Only one of --exclude-set and --include-set can be specified."),
                           ([], "Must provide a VCF file and/or aligned BAM file to perform diplotyping."),
                           (["--bam", VCF, "--max-error-rate", "2"], "--max-error-rate must be between 0.0 and 1.0")):
        out = run_cli(pkg, *base, *extra)
        assert out.returncode == 64 and message in out.stderr, (extra, out.stderr)
    # the reference options this implementation does not carry are refused by name
    for flag in (["--hla-revert-method"], ["--output-cyp2d6-bam", "x.bam"], ["--debug-hla-target", "HLA:HLA00001"]):
        out = run_cli(pkg, *base, "--vcf", VCF, *flag)
        assert out.returncode == 64 and flag[0] in out.stderr and "not supported" in out.stderr
    assert not (tmp_path / "out.json").exists()


def test_create_without_a_device_is_an_error(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pkg.StarphaseError) as e:
        pkg.database.Starphase(DB, None)
    assert e.value.code == pkg.ffi.SP_ERR_NO_DEVICE


def test_cli_without_a_device_fails_after_the_checks(pkg, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    fasta = tmp_path / "ref.fa"
    fasta.write_text(">chr1\nACGT\n")
    out = run_cli(pkg, "diplotype", "-d", DB, "-r", str(fasta), "-o", str(tmp_path / "out.json"), "--vcf", VCF)
    assert out.returncode == 69 and not (tmp_path / "out.json").exists()
