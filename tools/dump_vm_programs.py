"""Dump the expression-VM program of every plan in a fixed corpus.

    python tools/dump_vm_programs.py [--lib PATH] [--out FILE] [--jit FILE]

Builds each plan (gx_build only: no GPU, nothing bound or opened) and records
gx_debug_vm_program's text. tests/golden/vm_programs.json holds the result
and tests/test_vm_programs.py compares the product library against it, so a
change to the host expression compiler that moves an instruction, a
register, a constant or a fetch slot shows up as a text diff.

The golden file pins what the engine compiled BEFORE the three host
compilers became one: it was written with --lib pointing at a build of that
earlier engine (plus gx_debug_vm_program alone). Entries named in NEW_ENTRIES
are plans that engine compiled to a program its own kernel could not run;
they are recorded from the current engine. Regenerate with --keep-old to
refresh only those and leave every other entry as it is.

--jit also writes gx_debug_jit_source of every fused plan, for a one-off
comparison between two builds.
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import gxlib  # noqa: E402
from tests import test_vm_sites as S  # noqa: E402
from tests.test_wide_projection import wide_plan  # noqa: E402
from tidb_amd import plan as P  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "vm_programs.json")
# no parent golden: the earlier engine lowered ROUND into the join-aggregate
# probe, whose kernel has no rounding, and wiped the third operand (ins.c) of
# the probe's VM_CMP / VM_IF along with the loads' fetch slots
NEW_ENTRIES = ("q3_round", "q3_if")

DEC, I64 = gxlib.GX_TYPE_DECIMAL, gxlib.GX_TYPE_I64


def _sites_plan(lib, group, kind):
    """tests/test_vm_sites.py's plan for `group`: a Projection, or
    sum(expr) GROUP BY g."""
    b = P.Builder(lib)
    src = b.source(S.TYPES, S.FRACS)
    exprs = S.GROUPS[group](b, False)
    if kind == "proj":
        root = b.projection(src, [e for e, _, _ in exprs])
    else:
        aggs = [(gxlib.GX_AGG_SUM,
                 e if t == DEC else b.call(gxlib.GX_F_CAST_DEC, DEC, 0, e), f)
                for e, t, f in exprs]
        root = b.hashagg(src, [b.colref(S.G, I64)], aggs)
    return b, root


def _year_key_plan(lib):
    """sum(a) GROUP BY YEAR(t): a computed group key in a stable register."""
    b = P.Builder(lib)
    src = b.source(S.TYPES, S.FRACS)
    year = b.call(gxlib.GX_F_YEAR, I64, 0, b.colref(S.T, gxlib.GX_TYPE_TIME))
    proj = b.projection(src, [year, b.colref(S.A, DEC, 2)])
    root = b.hashagg(proj, [b.colref(0, I64)],
                     [(gxlib.GX_AGG_SUM, b.colref(1, DEC, 2), 2)])
    return b, root


def _dec_key_plan(lib):
    """sum(a) GROUP BY b, b a decimal column: the key is a VM load."""
    b = P.Builder(lib)
    src = b.source(S.TYPES, S.FRACS)
    root = b.hashagg(src, [b.colref(S.B, DEC, 4)],
                     [(gxlib.GX_AGG_SUM, b.colref(S.A, DEC, 2), 2)])
    return b, root


def corpus():
    """name -> fn(lib) -> (builder, root)"""
    def named(fn, *args, **kw):  # plan.py's (builder, sources, root, ...)
        return lambda lib: (lambda r: (r[0], r[2]))(fn(lib, *args, **kw))

    plans = {
        "q1": named(P.q1_plan),
        "q3": named(P.q3_plan),
        "q3_round": named(P.q3_plan, limit=100000,
                          wrap_revenue=P.round_revenue),
        "q3_if": named(P.q3_plan, limit=100000, wrap_revenue=P.if_revenue),
        "wide": named(wide_plan),
        "year_key": _year_key_plan,
        "dec_key": _dec_key_plan,
    }
    for g in S.GROUPS:
        plans[f"agg_{g}"] = lambda lib, g=g: _sites_plan(lib, g, "agg")
        if g != "div":
            plans[f"proj_{g}"] = lambda lib, g=g: _sites_plan(lib, g, "proj")
    return plans


def declare(lib):
    lib.gx_debug_vm_program.restype = ctypes.c_char_p
    lib.gx_debug_vm_program.argtypes = [ctypes.c_void_p]
    lib.gx_debug_jit_source.restype = ctypes.c_char_p
    lib.gx_debug_jit_source.argtypes = [ctypes.c_void_p]
    return lib


def dump(lib, make_plan, jit=False):
    b, root = make_plan(lib)
    ex = b.build(root)
    text = lib.gx_debug_vm_program(ex.ex).decode()
    if jit:
        src = lib.gx_debug_jit_source(ex.ex).decode()
        text = src if text.startswith("site fused") else ""
    ex.free()
    b.free()
    return text


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="engine library (default: the product)")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--jit", help="also write the fused plans' kernel source")
    ap.add_argument("--keep-old", action="store_true",
                    help="rewrite only NEW_ENTRIES in an existing --out")
    args = ap.parse_args()
    lib = declare(gxlib._decl(ctypes.CDLL(args.lib)) if args.lib
                  else gxlib.load_product())
    plans = corpus()
    out = {}
    if args.keep_old:
        with open(args.out) as f:
            out = json.load(f)
        plans = {n: plans[n] for n in NEW_ENTRIES}
    for name, make_plan in plans.items():
        out[name] = dump(lib, make_plan)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    if args.jit:
        with open(args.jit, "w") as f:
            json.dump({n: dump(lib, p, jit=True) for n, p in plans.items()},
                      f, indent=1, sort_keys=True)
    print(f"{len(plans)} programs -> {args.out}")


if __name__ == "__main__":
    main()
