"""The k-loop schedule of split_pingpong_kernel (exprgrad_amd/csrc/kernels/split_schedule.hpp) on the CPU: the header the
kernel takes its barrier counts, vmcnt values and stage numbers from, replayed for the eight waves of a block barrier
generation by barrier generation (tests/split_schedule_driver.cpp).  For every KT the driver asserts that all waves meet
the same number of barriers, that every stage read is a barrier behind the issuers' wait that retires it, that no LDS-DMA
piece goes into a stage some wave may still read, that every vmcnt is exactly the pieces that may still fly, and that
every wave reads k-tiles 0 .. KT - 1 once each in order; and that three broken variants of the schedule are caught.  The
gate admits K >= 2048 only (KT >= 128): the small KT are here because the prologue and the tail go wrong there first."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KTS = [1, 2, 3, 4, 5, 6, 7, 128, 130, 132]


def test_pingpong_schedule_replayed_for_eight_waves(tmp_path):
    exe = str(tmp_path / "split_schedule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "split_schedule_driver.cpp"),
                           "-o", exe])
    out = subprocess.run([exe] + [str(k) for k in KTS], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ALL PASS", out.stdout + out.stderr
    assert [l.split()[:2] for l in lines[:-1]] == [["PASS", "KT=%d" % k] for k in KTS], out.stdout
