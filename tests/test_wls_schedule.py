"""S2's batch schedule (csrc/nct_wls_schedule.h: how many PCG iterations the host enqueues between two convergence polls, sized by a convergence forecast) on the CPU.
Results and iteration counts do not depend on the schedule, so no solver test notices when the forecast stops working; this one does."""
import os
import subprocess

import nct


def test_schedule_against_model_solver(tmp_path):
    """tests/wls_schedule_check.cpp drives the class with a model solver (geometric, stalling, already-solved and zero right-hand sides, iteration budgets) under
    AddressSanitizer + UBSan: the batch sizes, iterations enqueued / needed and snapshots read equal the ones recorded from the loop the class was taken out of, and a turn
    with nothing in flight and a forecast never gets an empty batch."""
    exe = str(tmp_path / "wls_schedule_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(nct.PKG_ROOT, "csrc"),
                        os.path.join(os.path.dirname(__file__), "wls_schedule_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["ok", "19"], r.stdout[-2000:] + r.stderr[-4000:]
