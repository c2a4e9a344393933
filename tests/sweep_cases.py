"""Case tables, input generators and the dispatch of the closed-shell XC sweep and the AO evaluation, restated
(tests/test_sweep_cases_cpu.py, tests/test_gpu_sweep_dispatch.py, tools/sweep_ledger_trace.py).

`expected_kernels(case)` says, in Python, which template instantiations of the families in LEDGER_KERNELS a case
launches: takes_tiny / plan_sweep / launch_density / vxc_stage / density_source / prepare_ao_table / launch_ao of
csrc/dft_api.hip, occ_plan / launch_nto of csrc/xc_occ.hip, launch_eval_ao_pt of csrc/ao_kernels.hpp.  The CPU suite
holds every instantiation in the compiler's resource report against these claims, both ways: a new instantiation needs a
new case, a retired one takes its cases along.  tools/sweep_ledger_trace.py holds the restatement against the kernel
names of a trace.

None of the template choices depends on the device's CU count: num_cu enters plan_sweep, tiny_workgroups, launch_nto and
launch_eval_ao_pt through grid sizes, slab counts and chunk lengths only (checked by reading those functions; the trace
tool would show a dependence as a difference on the device it runs on).

Constants come from the headers by regular expression: a changed constant moves the restatement, a renamed one fails
the import.
"""
import functools
import math
import os
import re
from collections import namedtuple

import numpy as np

import jk_cases

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quantum_compute_dft_amd", "csrc")


def _src(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _constants(text, names):
    """{name: value} of `constexpr int A = 1, B = A + 1;` declarations (integer expressions over earlier names)."""
    out = {}
    for decl in re.findall(r"constexpr\s+int\s+([^;]+);", text):
        for part in decl.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*([\w\s+*()-]+?)\s*", part)
            if m and all(t.isdigit() or t in out for t in re.findall(r"\w+", m.group(2))):   # (template parameters: skipped)
                out[m.group(1)] = int(eval(m.group(2), {"__builtins__": {}}, dict(out)))   # noqa: S307  (digits, names, + * -)
    missing = [n for n in names if n not in out]
    if missing:
        raise RuntimeError(f"constants {missing} not found: the restatement in tests/sweep_cases.py needs them")
    return {n: out[n] for n in names}


def _kb(text, pattern, what):
    m = re.search(pattern, text)
    if not m:
        raise RuntimeError(f"{what}: pattern {pattern!r} not found, restate it in tests/sweep_cases.py")
    return int(m.group(1)) * 1024


_occ_h, _occ_c, _ao_h, _api = _src("xc_occ_kernels.hpp"), _src("xc_occ.hip"), _src("ao_kernels.hpp"), _src("dft_api.hip")
globals().update(_constants(_occ_h, ["OC_KC", "OC_LDA", "OC_OT", "OC_OR"]))
globals().update(_constants(_ao_h, ["AO_CW", "AO_MAX_L"]))
globals().update(_constants(_src("xc_tiny_launch.hpp"), ["TINY_MAX_NAO"]))
OCC_RES_LIMIT = _kb(_occ_c, r"res_limit\s*=\s*(\d+)\s*\*\s*1024", "resident limit of occ_plan")                # 80 KB
AO_TAB_LIMIT = _kb(_ao_h, r"tile_b\s*\+\s*tab_b\s*<=\s*(\d+)\s*\*\s*1024", "shell-table limit of the AO launch")  # 64 KB
AO_PT_LIMIT = _kb(_api, r">\s*(\d+)\s*\*\s*1024\s*\?\s*8\s*:\s*16", "tile-height rule of launch_ao")            # 53 KB
_m = re.search(r"struct\s+AoShell\s*\{([^}]*)\}", _ao_h)
if not _m:
    raise RuntimeError("struct AoShell not found")
AO_SHELL_BYTES = sum({"double": 8, "int": 4}[t] * len(names.split(",")) for t, names in re.findall(r"(double|int)\s+([^;]+);", _m.group(1)))

# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
# entry  "xc": DFT_ComputeXC64 (dm);  "xc_occ": DFT_ComputeXCOcc (orbitals, dm = cocc cocc^T; `pass_dm` False: no dm);
#        "xc_direct": DFT_ComputeXCDirect on the shell table `table` in chunks of `chunk` points;  "eval_ao": DFT_EvalAO
#        on `table`, `xc` = "GGA" with gradient planes, "LDA" without.
# xc     "LDA", "GGA", "B3LYP", or the mix "pbe_x + pbe_c" (GGA's numbers through the mix solver)
# options: None leaves the library's default.  `aligned` False: every plane starts 8 bytes into its allocation.
# env    (("QCDFT_OCC_NW", "8"),): variables occ_plan reads with getenv at every plan (tools/occ_time.py sets them)
MIX = "pbe_x + pbe_c"
Case = namedtuple("Case", "entry xc ngrid nao nocc tiny path vxc_fringe occ ao_pt ksplit sweep_order aligned env seed note table chunk pass_dm",
                  defaults=(0, None, None, None, None, None, None, None, True, (), 0, "", None, 0, True))
NG = 16 * 64 + 5            # a ragged last 16-row sub-tile, more sub-tiles than one per wave
NG_BIG = 16 * 19 + 3        # nao > 128: a few hundred points
NG_AO = 43                  # AO tables out of LDS: three tiles of 16, six of 8, the last one ragged
FUNCS = ("LDA", "GGA", "B3LYP")

# the wave-specialised kernels k_rho_ws / k_vxc_ws: per tile count NT = ceil(nao / 16), (odd, even) widths that pad their
# last tile and, from NT = 2, the widths 16 (NT - 1) + 1..4 that take the fringe form of k_vxc_ws (LDA, GGA), both parities
WS_PLAIN = {1: (15, 16), 2: (23, 32), 3: (37, 48), 4: (55, 64), 5: (71, 80), 6: (87, 96), 7: (103, 112), 8: (119, 128)}
WS_FRINGE = {2: (17, 18), 3: (33, 35, 36), 4: (49, 51, 52), 5: (67, 66, 68), 6: (81, 83, 82, 84), 7: (99, 98), 8: (113, 115, 116)}
WS_CASES = ([Case("xc", xc, NG, nao, tiny=0, seed=1, note=f"NT = {nt}, padded last tile")
             for nt, ws in WS_PLAIN.items() for nao in ws for xc in FUNCS] +
            [Case("xc", xc, NG, nao, tiny=0, seed=2, note=f"NT = {nt}, fringe remainder {nao % 16}" + (" (declined: symmetrised slabs)" if xc == "B3LYP" else ""))
             for nt, ws in WS_FRINGE.items() for nao in ws for xc in FUNCS if xc != "B3LYP" or nao in (33, 82, 113)] +
            [Case("xc", xc, NG, nao, tiny=0, vxc_fringe=0, seed=3, note="fringe width on the padded grid") for nao in (49, 66) for xc in ("LDA", "GGA")] +
            [Case("xc", "GGA", NG, 3, tiny=0, seed=4, note="narrowest: three functions in one tile"),
             Case("xc", "LDA", 5, 1, tiny=0, seed=5, note="one function, fewer points than a sub-tile"),
             Case("xc", "GGA", NG, 82, tiny=0, sweep_order=3, seed=6, note="both kernels walk the grid from its end"),
             Case("xc", "B3LYP", NG, 52, tiny=0, sweep_order=3, seed=7, note="walking order with symmetrised slabs"),
             Case("xc", "GGA", NG, 52, tiny=0, aligned=False, seed=8, note="even nao, planes 8 bytes off: VEC = false, fringe"),
             Case("xc", "LDA", NG, 96, tiny=0, aligned=False, seed=9, note="even nao, plane 8 bytes off: VEC = false"),
             Case("xc", MIX, NG, 52, seed=10, note="mix solver on the GGA kernels, fringe"),
             Case("xc", MIX, NG, 24, seed=11, note="a mix never takes the one-kernel sweep")])
TINY_CASES = ([Case("xc", xc, NG, nao, seed=12, note="one-kernel sweep, " + ("one tile" if nao <= 16 else "two tiles"))
               for nao in (9, 16, 17, 32) for xc in FUNCS] +
              [Case("xc", "GGA", NG, 33, seed=13, note="first width past the one-kernel sweep"),
               Case("xc", "LDA", 7, 2, seed=14, note="one-kernel sweep, fewer points than a sub-tile"),
               Case("xc", "B3LYP", NG, 32, tiny=1, seed=15, note="one-kernel sweep forced")])
BIG_CASES = ([Case("xc", xc, NG_BIG, nao, seed=16, note="tiled kernels, " + ("8-byte" if nao % 2 else "16-byte") + " loads")
              for nao in (129, 130) for xc in FUNCS] +
             [Case("xc", "GGA", NG_BIG, 130, aligned=False, seed=17, note="tiled kernels, even nao, planes 8 bytes off"),
              Case("xc", "B3LYP", 2 * NG_BIG, 150, ksplit=3, seed=18, note="ksplit has no say over the split-K of nao > 128")])
PATH_CASES = ([Case("xc", xc, NG, 37, path=p, seed=19, note=("plain-VALU" if p == 1 else "generic MFMA") + " kernels")
               for p in (1, 2) for xc in FUNCS] +
              [Case("xc", "GGA", NG_BIG, 150, path=2, ksplit=3, seed=20, note="generic MFMA kernels, three grid chunks, 2 x 2 blocks"),
               Case("xc", "B3LYP", NG_BIG, 131, path=1, seed=21, note="plain-VALU kernels past 128 functions")])

# occupied-orbital density kernels.  (nao, nocc) per orbital-tile count NTO: resident (all of C in LDS, k_rho_occ_rs), at its
# limit of nao where that is above nocc; more than one chunk per wave (MULTI: nao > 128); streamed (k_rho_occ, four waves)
_RS = {1: ((40, 9), (41, 16), (128, 12), (129, 12), (384, 16), (161, 5)), 2: ((50, 20), (51, 32), (192, 17), (161, 30)),
       3: ((96, 40), (81, 33)), 4: ((64, 64), (63, 49))}
_STREAM4 = {1: ((385, 16), (386, 3)), 2: ((193, 32), (194, 17)), 3: ((97, 48), (98, 33)), 4: ((65, 49), (66, 64))}
_STREAM8 = {5: ((81, 65), (90, 80)), 6: ((97, 81), (100, 96)), 7: ((113, 97), (120, 112)), 8: ((127, 113), (128, 128)),
            "two passes": ((140, 129), (141, 130))}
# MULTI at NTO = 3, 4 needs five chunks of C (nao > 128) in LDS: above the default 80 KB, reachable through
# QCDFT_OCC_RES_KB alone (tools/occ_time.py), like the eight-wave streamed kernels at NTO <= 4 through QCDFT_OCC_NW
_RS_ENV = {3: ((130, 40, "100"), (131, 48, "100")), 4: ((130, 64, "128"), (133, 50, "128"))}


def _ng(nao):
    return NG if nao <= 128 else NG_BIG


OCC_CASES = ([Case("xc_occ", xc, _ng(nao), nao, nocc, occ=1, seed=22, note=f"NTO = {nto}, C resident" + (", MULTI" if nao > 128 else ""))
              for nto, shapes in _RS.items() for nao, nocc in shapes for xc in ("LDA", "GGA")] +
             [Case("xc_occ", xc, NG_BIG, nao, nocc, occ=1, env=(("QCDFT_OCC_RES_KB", kb),), seed=23, note=f"NTO = {nto}, MULTI with a raised resident limit")
              for nto, shapes in _RS_ENV.items() for nao, nocc, kb in shapes for xc in ("LDA", "GGA")] +
             [Case("xc_occ", xc, _ng(nao), nao, nocc, occ=1, seed=24, note=f"NTO = {nto}, streamed, four waves")
              for nto, shapes in _STREAM4.items() for nao, nocc in shapes for xc in ("LDA", "GGA")] +
             [Case("xc_occ", xc, _ng(nao), nao, nocc, occ=1, env=(("QCDFT_OCC_NW", "8"),), seed=25, note=f"NTO = {nto}, streamed, eight waves by QCDFT_OCC_NW")
              for nto, shapes in _STREAM4.items() for nao, nocc in shapes for xc in ("LDA", "GGA")] +
             [Case("xc_occ", xc, _ng(nao), nao, nocc, occ=1, seed=26, note=f"NTO = {nto}, streamed, eight waves")
              for nto, shapes in _STREAM8.items() for nao, nocc in shapes for xc in ("LDA", "GGA")] +
             [Case("xc_occ", "B3LYP", NG, 114, 21, seed=27, note="automatic choice: the occupied form pays"),
              Case("xc_occ", "GGA", NG, 114, 21, pass_dm=False, seed=28, note="automatic choice, no dm handed over"),
              Case("xc_occ", "GGA", NG, 36, 21, pass_dm=False, seed=29, note="automatic choice: the dm form, dm built from the orbitals"),
              Case("xc_occ", "B3LYP", NG, 36, 21, occ=2, seed=30, note="occupied form switched off"),
              Case("xc_occ", "GGA", NG, 24, 5, seed=31, note="the one-kernel sweep has no occupied form"),
              Case("xc_occ", "GGA", NG, 64, 33, occ=1, aligned=False, seed=32, note="resident C, even nao, planes 8 bytes off"),
              Case("xc_occ", "LDA", NG, 98, 40, occ=1, aligned=False, seed=33, note="streamed, even nao, plane 8 bytes off"),
              Case("xc_occ", "B3LYP", NG_BIG, 200, 40, occ=1, seed=34, note="streamed past 128 functions, tiled Vxc kernels")])

SWEEP_CASES = WS_CASES + TINY_CASES + BIG_CASES + PATH_CASES + OCC_CASES

# AO evaluation.  TAB = false (the shell table does not fit beside the tile in LDS) needs hundreds of shells; `ao_pt` None
# is the automatic tile height.  xc "GGA": values and gradients, "LDA": values alone.
AO_CASES = ([Case("eval_ao", xc, NG_AO, 0, table=t, ao_pt=pt, seed=40, note="shell table in global memory")
             for t in ("huge_even", "huge_odd") for xc in ("GGA", "LDA") for pt in (8, 16)] +
            [Case("eval_ao", xc, NG_AO, 0, table=t, ao_pt=pt, seed=41, note="shell table in LDS")
             for t in ("t84", "t83") for xc in ("GGA", "LDA") for pt in (8, 16)] +
            [Case("eval_ao", "GGA", NG_AO, 0, table="huge_even", seed=42, note="automatic tile height with gradients: 8"),
             Case("eval_ao", "LDA", NG_AO, 0, table="big_even", seed=43, note="automatic tile height without gradients: 16, table out of LDS"),
             Case("eval_ao", "GGA", NG_AO, 0, table="borrow", seed=44, note="block seam on an odd column: the previous shell moves over"),
             Case("eval_ao", "GGA", NG_AO, 0, table="t130", aligned=False, seed=45, note="even nao, outputs 8 bytes off: 8-byte stores"),
             Case("eval_ao", "GGA", NG_AO, 0, table="t37", seed=46, note="one block, automatic tile height 16")])
# (table, with gradients): tile heights 16 and 8 put the same table out of and into LDS -- bitwise equal outputs
AO_TAB_PAIRS = [("mid_even", True), ("mid_odd", True), ("big_even", False)]

DIRECT_CASES = [
    Case("xc_direct", "GGA", NG, 0, table="t37", chunk=256, seed=50, note="odd nao, wave-specialised; ragged last chunk of 5 points, gradient planes 8 bytes off"),
    Case("xc_direct", "LDA", NG, 0, table="t37", chunk=512, seed=51, note="values alone; chunks of 512, 512, 5"),
    Case("xc_direct", "B3LYP", 1024, 0, table="t37", chunk=256, seed=52, note="chunks divide the grid"),
    Case("xc_direct", "GGA", NG, 0, table="t83", chunk=300, seed=53, note="fringe width; 300 rounds up to 512"),
    Case("xc_direct", "B3LYP", NG, 0, table="t83", chunk=4096, seed=54, note="chunk larger than the grid"),
    Case("xc_direct", "GGA", 2 * NG_BIG + 256, 0, table="t130", chunk=256, seed=55, note="tiled kernels, two AO column blocks, ragged last chunk"),
    Case("xc_direct", "B3LYP", NG_BIG, 0, table="t130", chunk=0, seed=56, note="tiled kernels, automatic chunk (the whole grid)"),
    Case("xc_direct", "LDA", 2 * NG_BIG, 0, table="t130", chunk=256, seed=57, note="tiled kernels, values alone"),
]

ALL_CASES = SWEEP_CASES + AO_CASES + DIRECT_CASES


def case_id(c):
    s = f"{c.entry}-{c.xc.replace(' ', '')}-g{c.ngrid}"
    s += f"-{c.table}" if c.table else f"-n{c.nao}"
    if c.nocc:
        s += f"-o{c.nocc}"
    for k in ("tiny", "path", "vxc_fringe", "occ", "ao_pt", "ksplit", "sweep_order"):
        if getattr(c, k) is not None:
            s += f"-{k}{getattr(c, k)}"
    if c.chunk:
        s += f"-chunk{c.chunk}"
    if not c.aligned:
        s += "-unaligned"
    if not c.pass_dm:
        s += "-nodm"
    for k, v in c.env:
        s += f"-{k[6:]}{v}"
    return s


def options(c):
    """{option: value} to set on the solver of case `c`."""
    return {k: getattr(c, k) for k in ("tiny", "path", "vxc_fringe", "occ", "ao_pt", "ksplit", "sweep_order") if getattr(c, k) is not None}


def oracle_type(xc):
    return {"LDA": 0, "GGA": 1, "B3LYP": 2, MIX: 1}[xc]


# ---------------------------------------------------------------------------------------------------------------------
# dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------
def nt_of(nao):
    return -(-nao // 16)


def takes_tiny(c, nao):
    tiny = -1 if c.tiny is None else c.tiny
    return (c.path or 0) == 0 and tiny != 0 and c.xc != MIX and nao <= TINY_MAX_NAO      # planes stay far below 4 GiB here


def fringe(c, nao):
    """vxc_stage: the one-sided wave-specialised kernels take the fringe form at nao = 16 k + 1..4, k >= 1."""
    vf = -1 if c.vxc_fringe is None else c.vxc_fringe
    return (c.path or 0) == 0 and nao <= 128 and c.xc != "B3LYP" and vf != 0 and nao > 16 and 1 <= nao % 16 <= 4


def occ_rs_lds_bytes(nto, nch):
    yw = max(nto * 256, 16 * OC_LDA)
    return 8 * (nch * OC_KC * (16 * nto + 1) + 4 * yw + 2 * 4 * 16 * 3 + OC_OR * 16 * 4)


OccPlan = namedtuple("OccPlan", "npass nto nch resident nw multi mfma_occ mfma_full")


def occ_plan(nao, nocc, gga, env=()):
    env = dict(env)
    ntiles = -(-nocc // 16)
    npass = -(-ntiles // 8)
    nto = -(-ntiles // npass)
    nch = -(-nao // OC_KC)
    limit = int(env["QCDFT_OCC_RES_KB"]) * 1024 if "QCDFT_OCC_RES_KB" in env else OCC_RES_LIMIT
    resident = npass == 1 and nto <= 4 and occ_rs_lds_bytes(nto, nch) <= limit
    nw = 4 if (resident or nto <= 4) else 8
    if "QCDFT_OCC_NW" in env:
        nw = 4 if resident else (4 if int(env["QCDFT_OCC_NW"]) == 4 and nto <= 4 else 8)
    return OccPlan(npass, nto, nch, resident, nw, resident and nch > 4, npass * nch * 8.0 * nto * (2.0 if gga else 1.0), 4.0 * nt_of(nao) ** 2)


def resident_limit(nto):
    """Widest nao whose orbitals stay in LDS at `nto` orbital tiles, under the default limit."""
    nch = 0
    while occ_rs_lds_bytes(nto, nch + 1) <= OCC_RES_LIMIT:
        nch += 1
    return nch * OC_KC


def uses_occ(c, nao):
    if c.entry != "xc_occ" or takes_tiny(c, nao) or (c.path or 0) != 0 or c.occ == 2:
        return False
    p = occ_plan(nao, c.nocc, c.xc != "LDA", c.env)
    return c.occ == 1 or p.mfma_occ <= 0.85 * p.mfma_full


def sweep_kernels(c, nao, vec):
    """Kernels of one sweep over planes of `nao` columns; `vec`: 16-byte plane loads (even nao, aligned planes)."""
    G, S = c.xc != "LDA", c.xc == "B3LYP"
    path = c.path or 0
    fast, big = path == 0 and nao <= 128, path == 0 and nao > 128
    nt = nt_of(nao)
    out = set()
    if takes_tiny(c, nao):
        out.add(("k_sweep_tiny", (1 if nao <= 16 else 2, oracle_type(c.xc) if not S else 2, S)))
    else:
        if uses_occ(c, nao):
            p = occ_plan(nao, c.nocc, G, c.env)
            out.add(("k_rho_occ_rs", (p.nto, G, vec, p.multi)) if p.resident else ("k_rho_occ", (p.nto, p.nw, G, vec, False, 1)))
        elif fast:
            out.add(("k_rho_ws", (nt, G, vec)))
        elif big:
            out.add(("k_rho_big64", (G, vec)))
        else:
            out.add(("k_rho_valu" if path == 1 else "k_rho_mfma", (G,)))
        if fast:
            fr = fringe(c, nao)
            out.add(("k_vxc_ws", (nt, G, vec, S and not fr, fr)))
        elif big:
            out.add(("k_vxc_big", (G, vec)))
        else:
            out.add(("k_vxc_valu" if path == 1 else "k_vxc_mfma", (G,)))
    # the slab reduce (ground-state sweep): B3LYP past 128 functions reduces plainly and symmetrises after; B3LYP on the
    # generic kernels symmetrises in the reduce; everything else finishes Exc in the reduce
    out.add(("k_reduce_slabs8", (False, False) if S and big else (True, False) if S and not fast else (False, True)))
    return out


def ao_blocks(l):
    """prepare_ao_table: column blocks [(shell_lo, shell_hi, col_lo, ncol)] of shells of angular momenta `l`, and how many
    seams took the previous shell along to start on an even column."""
    blocks, col, borrowed = [], 0, 0
    for i, li in enumerate(l):
        nf = 2 * int(li) + 1
        if not blocks:
            blocks.append([i, i, col, 0])
        elif blocks[-1][3] + nf > AO_CW:
            b = blocks[-1]
            if col % 2 and b[1] - b[0] >= 2:
                pf = 2 * int(l[i - 1]) + 1
                b[1] -= 1
                b[3] -= pf
                blocks.append([i - 1, i, col - pf, pf])
                borrowed += 1
            else:
                blocks.append([i, i, col, 0])
        blocks[-1][1] = i + 1
        blocks[-1][3] += nf
        col += nf
    return [tuple(b) for b in blocks], borrowed


def ao_tab_bytes(sh):
    return AO_SHELL_BYTES * sh.nshell + 2 * 8 * len(sh.exp) + 4 * sh.nshell + 8


def ao_kernel(sh, grad, ao_pt, aligned):
    """launch_ao + launch_eval_ao_pt: (GRAD, VEC, PT, TAB) for the table `sh`."""
    blocks, _ = ao_blocks(sh.l)
    maxcol = max(b[3] for b in blocks)
    even = all(b[2] % 2 == 0 for b in blocks)
    vec = even and sh.nao % 2 == 0 and aligned
    planes = 4 if grad else 1
    pt = ao_pt or (8 if planes * 16 * (maxcol | 1) * 8 > AO_PT_LIMIT else 16)
    tab = 8 * planes * pt * (maxcol | 1) + ao_tab_bytes(sh) <= AO_TAB_LIMIT
    return ("k_eval_ao", (grad, vec, pt, tab))


def direct_chunks(c, num_cu=256):
    """DFT_ComputeXCDirect: points per chunk.  The automatic size (chunk = 0) is at least 1024 points per CU: the whole
    grid at these sizes on any device."""
    sh = ao_table(c.table)
    nplane = 1 if c.xc == "LDA" else 4
    chunk = c.chunk if c.chunk > 0 else max(int(96.0e6 / (8.0 * sh.nao * nplane)), 1024 * num_cu)
    chunk = min(-(-chunk // 256) * 256, c.ngrid)
    return [min(chunk, c.ngrid - g0) for g0 in range(0, c.ngrid, chunk)]


def expected_kernels(c):
    """Set of (kernel name, template arguments) of the families in LEDGER_KERNELS that case `c` launches."""
    if c.entry in ("xc", "xc_occ"):
        return sweep_kernels(c, c.nao, c.nao % 2 == 0 and c.aligned)
    sh = ao_table(c.table)
    grad = c.xc != "LDA"
    if c.entry == "eval_ao":
        return {ao_kernel(sh, grad, c.ao_pt, c.aligned)}
    if c.entry == "xc_direct":
        out = set()
        for n in direct_chunks(c):
            # the gradient planes lie n * nao doubles behind the values of the chunk: 16-byte aligned when that is even
            planes_aligned = not grad or (n * sh.nao) % 2 == 0
            out.add(ao_kernel(sh, grad, c.ao_pt, planes_aligned))
            out |= sweep_kernels(c._replace(entry="xc"), sh.nao, sh.nao % 2 == 0 and planes_aligned)
        return out
    raise ValueError(c.entry)


_ORDER = ("k_eval_ao", "k_sweep_tiny", "k_rho_occ_rs", "k_rho_occ", "k_rho_ws", "k_rho_big64", "k_rho_mfma", "k_rho_valu",
          "k_vxc_ws", "k_vxc_big", "k_vxc_mfma", "k_vxc_valu", "k_reduce_slabs8")


def launch_sequence(c):
    """The launches of `c` in stream order, ledger families only: what a kernel trace of the case shows."""
    in_order = lambda ks: sorted(ks, key=lambda k: _ORDER.index(k[0]))
    if c.entry != "xc_direct":
        return in_order(expected_kernels(c))
    sh, grad, out = ao_table(c.table), c.xc != "LDA", []
    for n in direct_chunks(c):
        planes_aligned = not grad or (n * sh.nao) % 2 == 0
        out.append(ao_kernel(sh, grad, c.ao_pt, planes_aligned))
        out += in_order(sweep_kernels(c._replace(entry="xc"), sh.nao, sh.nao % 2 == 0 and planes_aligned))
    return out


LEDGER_KERNELS = ("k_vxc_ws", "k_rho_ws", "k_rho_occ", "k_rho_occ_rs", "k_eval_ao", "k_sweep_tiny", "k_rho_big64", "k_vxc_big",
                  "k_rho_mfma", "k_vxc_mfma", "k_rho_valu", "k_vxc_valu", "k_reduce_slabs8")
# instantiations per family when this ledger was written: a floor, so that a report that no longer parses cannot pass
LEDGER_FLOOR = {"k_vxc_ws": 76, "k_rho_ws": 32, "k_rho_occ": 48, "k_rho_occ_rs": 32, "k_eval_ao": 16, "k_sweep_tiny": 6,
                "k_rho_big64": 4, "k_vxc_big": 4, "k_rho_mfma": 2, "k_vxc_mfma": 2, "k_rho_valu": 2, "k_vxc_valu": 2,
                "k_reduce_slabs8": 3}


def parse_instantiation(name):
    """(kernel name, template arguments) of a demangled kernel name, None for kernels outside LEDGER_KERNELS."""
    return jk_cases.parse_instantiation(name, LEDGER_KERNELS)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep_inputs(c):
    """(cocc, dm, ao, grad, w) of a sweep case: the recipe of tests/test_gpu_occ.occ_inputs (ao = 0.4 N, grad = 0.3 N,
    w = 0.05 U, cocc = sqrt(2) 0.7 N, dm = cocc cocc^T).  Read-only: shared between tests."""
    rng = np.random.default_rng(810000 + 1000 * c.seed + c.nao)
    nocc = c.nocc or max(1, -(-c.nao // 5))
    ao = 0.4 * rng.standard_normal((c.ngrid, c.nao))
    gr = 0.3 * rng.standard_normal((3, c.ngrid, c.nao))
    w = 0.05 * rng.random(c.ngrid)
    cocc = math.sqrt(2.0) * 0.7 * rng.standard_normal((c.nao, nocc))
    out = (cocc, cocc @ cocc.T, ao, gr, w)
    for a in out:
        a.setflags(write=False)
    return out


_CENTRES = np.array([[0.0, 0.0, 0.0], [2.1, 0.3, -0.4], [-1.7, 1.9, 0.6], [0.4, -2.3, 1.5], [1.2, 1.4, 2.6]])
# name: (shells, seed, first angular momenta).  Shells past the listed ones draw l from 0..3; the table ends with s / p / d
# shells that bring nao to the wanted width where one is given.
_TABLES = {"t37": (None, 37, 1, ()), "t83": (None, 83, 2, ()), "t84": (None, 84, 10, ()), "t130": (None, 130, 3, ()),
           "borrow": (None, 130, 4, (2,) * 25 + (1,)),          # 25 d shells end on column 125: the p shell does not fit, the seam is odd
           "mid_even": (80, None, 5, ()), "mid_odd": (80, None, 6, ()),
           "big_even": (318, None, 7, ()), "huge_even": (372, None, 8, ()), "huge_odd": (372, None, 9, ())}


@functools.lru_cache(maxsize=None)
def ao_table(name):
    """Synthetic basis.ShellTable: shells of l = 0..3 with 1..12 primitives (exponents 0.12..60, log-uniform) on five
    centres.  Names ending in _even / _odd get one more s shell where nao has the other parity."""
    from eri_fixtures import shell_table
    nshell, nao, seed, first = _TABLES[name]
    rng = np.random.default_rng(5200 + seed)
    l = list(first)
    if nao is not None:
        while nao - sum(2 * x + 1 for x in l) > 7:
            l.append(int(rng.integers(0, 4)))
        rest = nao - sum(2 * x + 1 for x in l)
        for x in (2, 1, 0, 0, 0):
            if rest >= 2 * x + 1:
                l.append(x)
                rest -= 2 * x + 1
        assert rest == 0
    else:
        l += [int(x) for x in rng.integers(0, 4, nshell - len(l))]
        if (sum(2 * x + 1 for x in l) % 2 == 0) != name.endswith("_even"):
            l.append(0)
    nprim = rng.integers(1, 13, len(l)) if nao is not None else rng.integers(3, 13, len(l))
    exp = np.exp(rng.uniform(np.log(0.12), np.log(60.0), int(nprim.sum())))
    coef = rng.uniform(0.3, 1.0, int(nprim.sum()))
    centre = _CENTRES[np.arange(len(l)) % len(_CENTRES)]
    return shell_table(centre, l, nprim, exp, coef)


@functools.lru_cache(maxsize=None)
def grid_inputs(c):
    """(coords, w, dm) of an AO or direct case: points around the five centres (sigma 1.3 bohr), the first five ON them."""
    sh = ao_table(c.table)
    rng = np.random.default_rng(820000 + 1000 * c.seed)
    coords = _CENTRES[rng.integers(0, len(_CENTRES), c.ngrid)] + 1.3 * rng.standard_normal((c.ngrid, 3))
    coords[:5] = _CENTRES
    w = 0.02 * rng.random(c.ngrid)
    C = 0.3 * rng.standard_normal((sh.nao, max(1, sh.nao // 6)))
    out = (coords, w, 2.0 * C @ C.T)
    for a in out:
        a.setflags(write=False)
    return out


def clear_caches():
    for f in (sweep_inputs, ao_table, grid_inputs):
        f.cache_clear()


@functools.lru_cache(maxsize=None)
def sweep_reference(c):
    """(Exc, Vxc) of the oracle for a sweep case: computed once, shared, read-only."""
    import oracle
    cocc, dm, ao, gr, w = sweep_inputs(c)
    exc, v = oracle.compute_xc(oracle_type(c.xc), dm, ao, w, gr if c.xc != "LDA" else None)
    v.setflags(write=False)
    return exc, v
