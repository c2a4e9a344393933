"""The restated sweep / AO dispatch of tests/sweep_cases.py against the kernels a device really launches.

    python tools/sweep_ledger_trace.py [--out profiles/sweep_ledger_trace.txt] [--timeout 600]

starts ONE fresh child under `rocprofv3 --kernel-trace` (no counters, no other tracing; the program goes after `--`).
The child runs every sweep, AO and direct case of the tables once, in table order, with a marker launch (a 2 x 2
DFT_ComputeCoulomb: k_jk_stream, a kernel no case launches) behind each.  The parent reads the kernel names of the
trace, cuts them at the markers and compares the launches of the ledger families, case by case and in order, with
sweep_cases.launch_sequence().  A tool, not a test: the coverage ledger of tests/test_sweep_cases_cpu.py is only as true as
expected_kernels(), and this is where that is held against the hardware.  On a disagreement the restatement or the
case table is what gets fixed, unless the dispatch itself is wrong.
"""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sweep_cases as sc  # noqa: E402

MARKER = "k_jk_stream"


def child():
    import numpy as np
    import torch
    import quantum_compute_dft_amd as q
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)

    def place(a, aligned):
        if aligned:
            return t(a)
        return torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), t(a).reshape(-1)])[1:].view(a.shape)

    marker = q.DFTSolverWrapper(q.library_path(), "LDA")
    m_eri, m_dm, m_j = (torch.ones((4, 4), dtype=torch.float64, device=dev), torch.ones((2, 2), dtype=torch.float64, device=dev),
                        torch.zeros((2, 2), dtype=torch.float64, device=dev))
    for c in sc.ALL_CASES:
        saved = {k: os.environ.get(k) for k, _ in c.env}
        os.environ.update(dict(c.env))
        s = q.DFTSolverWrapper(q.library_path(), c.xc)
        for k, v in sc.options(c).items():
            s.set_option(k, v)
        gga = c.xc != "LDA"
        if c.entry in ("xc", "xc_occ"):
            cocc, dm, ao, gr, w = sc.sweep_inputs(c)
            d_ao, d_gr = place(ao, c.aligned), (place(gr, c.aligned) if gga else None)
            d_v = torch.zeros((c.nao, c.nao), dtype=torch.float64, device=dev)
            if c.entry == "xc":
                s.compute_xc(c.ngrid, c.nao, t(dm), d_ao, t(w), d_v, d_gr)
            else:
                s.compute_xc_occ(c.ngrid, c.nao, cocc.shape[1], t(cocc), d_ao, t(w), d_v, d_gr, t(dm) if c.pass_dm else None)
        else:
            sh = sc.ao_table(c.table)
            coords, w, dm = sc.grid_inputs(c)
            if c.entry == "eval_ao":
                d_ao = place(np.zeros((c.ngrid, sh.nao)), c.aligned)
                d_gr = place(np.zeros((3, c.ngrid, sh.nao)), c.aligned) if gga else None
                s.eval_ao(sh, t(coords), c.ngrid, d_ao, d_gr)
            else:
                d_v, d_e = torch.zeros((sh.nao, sh.nao), dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
                s.compute_xc_direct(sh, c.ngrid, t(coords), t(w), t(dm), d_v, d_e, c.chunk)
        torch.cuda.synchronize()
        marker.compute_coulomb(2, m_eri, m_dm, m_j)
        torch.cuda.synchronize()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        del s
    print("child: ran", len(sc.ALL_CASES), "cases")


def read_trace(folder):
    """[[(kernel, template arguments) ...] per stretch between markers] of the newest kernel trace under `folder`."""
    files = sorted(glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel trace under {folder}")
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    groups, cur, in_marker = [], [], False
    for r in rows:
        name = re.sub(r"\((?:int|bool)\)", "", r["Kernel_Name"])
        if not name.startswith("void "):
            name = "void " + name
        if "qcdft::" + MARKER + "<" in name:
            if not in_marker:
                groups.append(cur)
                cur = []
            in_marker = True
            continue
        k = sc.parse_instantiation(name)
        if k is not None:
            cur.append(k)
            in_marker = False
    return groups, cur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_ledger_trace.txt"))
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    if a.child:
        return child()
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child"]
        rc = subprocess.run(cmd, timeout=a.timeout, cwd=ROOT).returncode        # a fresh process; ended at the time limit
        if rc != 0:
            raise SystemExit(f"the traced child ended with status {rc}: nothing compared")
        groups, tail = read_trace(tmp)
    lines = ["# Kernels launched per case (rocprofv3 --kernel-trace of tools/sweep_ledger_trace.py, ledger families only) against",
             "# sweep_cases.launch_sequence(): the restated dispatch of tests/sweep_cases.py held against the device."]
    bad = 0
    if len(groups) != len(sc.ALL_CASES) or tail:
        bad += 1
        lines.append(f"DIFFERENT: {len(groups)} marked stretches for {len(sc.ALL_CASES)} cases, {len(tail)} launches behind the last marker")
    seen = set()
    for c, got in zip(sc.ALL_CASES, groups):
        want = sc.launch_sequence(c)
        seen |= set(got)
        if got != want:
            bad += 1
            lines.append(f"DIFFERENT {sc.case_id(c)}\n    restated: {want}\n    launched: {got}")
    claimed = {k for c in sc.ALL_CASES for k in sc.expected_kernels(c)}
    lines.append(f"cases: {len(sc.ALL_CASES)}   differing: {bad}   instantiations launched: {len(seen)}   claimed: {len(claimed)}   claimed and not launched: {sorted(claimed - seen)}")
    if not bad:
        lines.append("agreement: every case launched exactly the kernels the restatement names, in its order")
        for fam in sc.LEDGER_KERNELS:
            lines.append(f"  {fam:18s} {sum(1 for k in seen if k[0] == fam):3d} instantiations launched")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
