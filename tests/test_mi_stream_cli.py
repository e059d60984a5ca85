"""mi-stream command line, CPU side: every path that returns before the
first HIP call — usage, --help, the range checks of --memtest and
--gemmtest, and the two host-only dumps. The expected stdout, stderr and
exit status were recorded from the binary before main() was split into
parse / validate / dispatch, so they pin that split to the old behaviour."""

import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
MI_STREAM = REPO / "native" / "bin" / "mi-stream"

USAGE = (
    "mi-stream [--mib N] [--iters N] [--device D] [--no-mfma] [--tune]"
    " [--lds-compare] [--all-gpus] [--burn SECONDS] [--memtest [--passes N]"
    " [--vram-percent P] [--memtest-inject N]] [--memtest-pattern-dump"
    " PATTERN SEED INVERT CELL_OFFSET N_CELLS] [--gemmtest [--gemm-size S |"
    " --gemm-mnk M N K] [--gemm-iters I | --gemm-seconds T]"
    " [--gemm-inject N]] [--gemm-operand-dump WHICH SEED ROW0 COL0 ROWS"
    " COLS]\n")
MEMTEST_NEEDS = (
    "mi-stream: --memtest needs --passes >= 1, --mib >= 1, --vram-percent"
    " 1..90, --memtest-inject 1..16\n")
GEMMTEST_NEEDS = (
    "mi-stream: --gemmtest needs M and N multiples of 128, K a multiple of"
    " 64 and <= 32768, one of --gemm-iters >= 1 / --gemm-seconds >= 1,"
    " --gemm-inject 1..16\n")

# (arguments, exit status, stdout, stderr)
CASES = [
    ("--help", 0, USAGE, ""),
    ("--bogus", 2, USAGE, ""),
    ("--mib", 2, USAGE, ""),  # value missing
    ("--memtest --passes 0", 2, "", MEMTEST_NEEDS),
    ("--memtest --vram-percent 91", 2, "", MEMTEST_NEEDS),
    ("--memtest --memtest-inject 17", 2, "", MEMTEST_NEEDS),
    ("--gemmtest --gemm-size 100", 2, "", GEMMTEST_NEEDS),
    # K over the exactness bound
    ("--gemmtest --gemm-mnk 128 128 32832", 2, "", GEMMTEST_NEEDS),
    ("--gemmtest --gemm-iters 1 --gemm-seconds 1", 2, "", GEMMTEST_NEEDS),
    ("--gemmtest --gemm-inject 17", 2, "", GEMMTEST_NEEDS),
    ("--memtest-pattern-dump 3 0 0 0 1", 2, "",
     "mi-stream: unknown memtest pattern 3\n"),
    ("--gemm-operand-dump 2 0 0 0 1 1", 2, "",
     "mi-stream: operand WHICH must be 0 (A) or 1 (B)\n"),
    # flags are read left to right: whichever comes first wins
    ("--bogus --memtest-pattern-dump 0 0 0 0 1", 2, USAGE, ""),
    ("--memtest-pattern-dump 0 0 0 0 2 --bogus", 0,
     "00000000 ffffffff 00000000 00000000\n"
     "688990c0 97766f3f 32180d10 44c86034\n", ""),
]


@pytest.mark.parametrize("args,status,stdout,stderr", CASES,
                         ids=[c[0] for c in CASES])
def test_host_only_paths(args, status, stdout, stderr):
    """Runs without a GPU: each of these returns before any HIP call."""
    if not MI_STREAM.exists():
        pytest.skip("native/bin/mi-stream not built")
    proc = subprocess.run([str(MI_STREAM)] + args.split(),
                          capture_output=True, text=True, timeout=60)
    assert (proc.returncode, proc.stdout, proc.stderr) == \
        (status, stdout, stderr)
