"""Which form of the HIP QP kernel a problem shape runs, without a GPU: mpc_benchmark_amd/csrc/qp_layout.h (the rule mpc_qp_create applies) compiled
with g++ into tests/_native/qp_layout_dump.cpp and read back as a table.  tests/test_qp_layout.py checks the plans; tests/test_gpu_qp_planted.py
reads from the same table which kernel each of its creations launches."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024
FORMS = ((1, 1), (2, 1), (0, 1), (1, 0), (0, 0))  # (mats, mf): the five instantiations of k_qp_solve (csrc/qp_host.h qp_launch)
# the four ways a shape is created: (batch, MPC_QP_NO_MFMA set)
CREATIONS = ((6, False), (300, False), (6, True), (300, True))


def layout_table(shapes, exe_dir=None):
    """shapes: (n, neq, nin, box) -> {(n, neq, nin, box, batch, no_mfma): plan}, plan = dict of the header line's integers + "regions"
    {name: (start, length)} in doubles."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(exe_dir or tmp, "qp_layout_dump")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "_native", "qp_layout_dump.cpp")])
        args = [str(int(v)) for s in shapes for v in s[:4]]
        text = subprocess.check_output([exe] + args, text=True)
    table = {}
    for line in text.splitlines():
        head, regs = line.split(" | ")
        p = {k: int(v) for k, v in (kv.split("=") for kv in head.split())}
        p["regions"] = {name: (int(a), int(b)) for name, a, b in (r.split(":") for r in regs.split())}
        table[(p["n"], p["neq"], p["nin"], bool(p["box"]), p["batch"], not p["allow_mf"])] = p
    assert len(table) == 4 * len(set(tuple(s[:4]) for s in shapes))
    return table


def creations(table, shape):
    """The creations of one shape with the duplicates of the same (mats, mf) dropped: [(batch, no_mfma, (mats, mf))], CREATIONS order."""
    out, seen = [], set()
    for batch, no_mfma in CREATIONS:
        p = table[tuple(shape[:4]) + (batch, no_mfma)]
        form = (p["mats"], p["mf"])
        if form not in seen:
            seen.add(form)
            out.append((batch, no_mfma, form))
    return out
