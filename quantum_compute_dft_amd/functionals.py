"""Exchange-correlation functionals as weighted sums of the engine's eight pointwise components and its two meta-GGA
components (tpss_x, tpss_c: functions of the kinetic-energy density tau as well).

`resolve(spec)` turns a table name ("PBE0", case-insensitive) or an expression
("0.75*pbe_x + pbe_c + 0.25*hf") into a `Functional`.  Three names keep the reference's built-in
solver types (DFT_CreateSolver(0/1/2): same kernels, same results bit for bit); everything else runs
as a mix solver (DFT_CreateSolverMix), whose per-point sums follow the GGA convention described in
include/dft_solver.h.

The named recipes are the literature's definitions as far as they could be written down from memory; the
COMPOSITION is tested (against the oracle's own pieces), the recipes are not cross-checked against another
code.  "TPSS" / "TPSSH" are as recalled too: their exchange is pinned by the exact hydrogen-atom energy, their correlation by
its one-electron and slowly-varying limits (tests/test_meta_cpu.py).  "B3LYP" carries VWN-RPA (the reference's choice), "B3LYP5" carries VWN5.
"""
import math
import re
from collections import namedtuple

# ABI order: enum XCComponent of include/dft_solver.h = the oracle's pointwise kinds 0..7
COMPONENTS = ("slater_x", "vwn5_c", "vwn_rpa_c", "pw92_c", "pbe_x", "pbe_c", "b88_x", "lyp_c")
# spellings accepted in expressions and in the table below (the oracle's short names among them)
_ALIASES = {"slater": "slater_x", "vwn5": "vwn5_c", "vwn_rpa": "vwn_rpa_c", "pw92": "pw92_c", "b88": "b88_x", "lyp": "lyp_c"}
_GRADIENT = COMPONENTS[4:]
# ABI order: enum XCMetaComponent of include/dft_solver.h; a functional that carries one needs tau (DFT_CreateSolverMeta)
META_COMPONENTS = ("tpss_x", "tpss_c")
_QUIRKY = ("vwn5_c", "pbe_c")          # the two components option "quirks" changes


class Functional(namedtuple("Functional", "name weights c_hf builtin_type")):
    """weights: {component name: coefficient} (non-zero entries only); c_hf: exact-exchange fraction;
    builtin_type: 0/1/2 for the reference's three solver types, None for a mix solver."""
    __slots__ = ()

    @property
    def needs_gradient(self):
        return self.needs_tau or any(k in _GRADIENT for k in self.weights)

    @property
    def needs_tau(self):
        """A meta-GGA: the functional reads the kinetic-energy density."""
        return any(k in META_COMPONENTS for k in self.weights)

    @property
    def uses_quirks(self):
        return any(k in _QUIRKY for k in self.weights)

    @property
    def wants_k(self):
        return self.c_hf != 0.0

    def weight_vector(self):
        """The eight coefficients in ABI order."""
        return [float(self.weights.get(k, 0.0)) for k in COMPONENTS]

    def meta_weight_vector(self):
        """The coefficients of the meta-GGA components in ABI order."""
        return [float(self.weights.get(k, 0.0)) for k in META_COMPONENTS]


def _f(name, c_hf=0.0, builtin=None, **w):
    return Functional(name, {_ALIASES.get(k, k): float(v) for k, v in w.items()}, float(c_hf), builtin)


_B3 = dict(slater=0.80, b88=0.72, lyp=0.81)
TABLE = {f.name: f for f in (
    _f("LDA", builtin=0, slater=1, vwn5=1),
    _f("SVWN", builtin=0, slater=1, vwn5=1),
    _f("GGA", builtin=1, pbe_x=1, pbe_c=1),
    _f("PBE", builtin=1, pbe_x=1, pbe_c=1),
    _f("B3LYP", 0.2, builtin=2, vwn_rpa=0.19, **_B3),
    _f("SVWN-RPA", slater=1, vwn_rpa=1),
    _f("PW92", slater=1, pw92=1),
    _f("BLYP", slater=1, b88=1, lyp=1),
    _f("PBE0", 0.25, pbe_x=0.75, pbe_c=1),
    _f("B1LYP", 0.25, slater=0.75, b88=0.75, lyp=1),
    _f("BHANDHLYP", 0.5, slater=0.5, b88=0.5, lyp=1),
    _f("B3LYP5", 0.2, vwn5=0.19, **_B3),
)}
# The meta-GGA names, a table of their own beside the twelve above: resolve() knows both
META_TABLE = {f.name: f for f in (
    _f("TPSS", tpss_x=1, tpss_c=1),
    _f("TPSSH", 0.1, tpss_x=0.9, tpss_c=1),
)}

_TERM = re.compile(r"^(?:([^*]+)\*)?([A-Za-z_][A-Za-z0-9_]*)$")


def _parse(spec):
    weights, c_hf, seen = {}, 0.0, set()
    text = spec.replace(" ", "").replace("\t", "")
    if not text:
        raise ValueError("empty functional expression")
    # split at the + / - that start a term (not the sign of an exponent: 1e-3*pbe_x)
    terms = re.findall(r"[+-]?(?:[^+-]|(?<=[eE])[+-])+", text)
    if "".join(terms) != text:
        raise ValueError(f"cannot parse functional expression {spec!r}")
    for t in terms:
        sign = -1.0 if t[0] == "-" else 1.0
        m = _TERM.match(t.lstrip("+-"))
        if not m:
            raise ValueError(f"cannot parse term {t!r} of functional expression {spec!r}")
        try:
            c = sign * (float(m.group(1)) if m.group(1) is not None else 1.0)
        except ValueError:
            raise ValueError(f"bad coefficient in term {t!r} of functional expression {spec!r}") from None
        if not math.isfinite(c):
            raise ValueError(f"non-finite coefficient in term {t!r} of functional expression {spec!r}")
        name = m.group(2).lower()
        name = _ALIASES.get(name, name)
        if name != "hf" and name not in COMPONENTS and name not in META_COMPONENTS:
            raise ValueError(f"unknown component {m.group(2)!r} in functional expression {spec!r} "
                             f"(known: {', '.join(COMPONENTS + META_COMPONENTS)}, hf)")
        if name in seen:
            raise ValueError(f"component {name!r} appears twice in functional expression {spec!r}")
        seen.add(name)
        if name == "hf":
            c_hf = c
        elif c != 0.0:
            weights[name] = c
    if not weights:
        raise ValueError(f"functional expression {spec!r} has no density-functional component with a non-zero weight")
    return Functional(spec.strip(), weights, c_hf, None)


# What the open-shell refusals add: the open-shell ground state of a meta-GGA is built, but opt-in
OPEN_SHELL_META_HINT = ("the open-shell ground state is too, but only on request: scf.run_uks(..., meta=True) / the driver's "
                        "--open-shell-meta, which go through HipBackend.uks_meta_parts (DFT_ComputeXCMetaSpin)")

# What the closed-shell gradient refusals add: the nuclear gradient of a meta-GGA is built, but opt-in
META_GRADIENT_HINT = ("the closed-shell nuclear gradient is too, but only on request: gradients.nuclear_gradient(..., meta=True) / the "
                      "driver's --meta-gradient, which go through HipBackend.xc_gradient_meta (DFT_ComputeXCGradientMeta)")

# What the open-shell gradient refusals add: the nuclear gradient of an open-shell meta-GGA is built, but opt-in
OPEN_SHELL_META_GRADIENT_HINT = ("the open-shell nuclear gradient is too, but only on request: gradients.nuclear_gradient_uks(..., "
                                 "meta=True) / the driver's --open-shell-meta-gradient, which go through "
                                 "HipBackend.xc_gradient_meta_spin (DFT_ComputeXCGradientMetaSpin)")


def refuse_meta(spec, what, hint=None):
    """ValueError when `spec` is a meta-GGA: `what` (a sentence's subject) is built for LDA / GGA / hybrid functionals only.
    `hint`: a sentence added for the callers that have an opt-in way round."""
    f = resolve(spec)
    if f.needs_tau:
        raise ValueError(f"{what}: {f.name!r} is a meta-GGA (it reads the kinetic-energy density tau) and this feature is not built "
                         "for meta-GGA functionals -- only the closed-shell ground state is" + (f"; {hint}" if hint else ""))


def resolve(spec):
    """Functional of a table name or an expression; ValueError for anything else."""
    if isinstance(spec, Functional):
        return spec
    if not isinstance(spec, str):
        raise ValueError(f"functional must be a name or an expression, not {type(spec).__name__}")
    key = spec.strip().upper()
    if key in TABLE:
        return TABLE[key]
    if key in META_TABLE:
        return META_TABLE[key]
    try:
        return _parse(spec)
    except ValueError as e:
        raise ValueError(f"Unsupported functional type: {key!r} ({e}; table: {', '.join(list(TABLE) + list(META_TABLE))})") from None
