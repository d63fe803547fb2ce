"""The host expression compiler's output, pinned text for text (CPU).

tests/golden/vm_programs.json holds gx_debug_vm_program's dump of a fixed
corpus (tools/dump_vm_programs.py): Q1, Q3, the register-recycling wide
projection, every expression group of tests/test_vm_sites.py as an aggregate
and as a Projection, and the two group-key shapes that rely on a stable
register. It was written by the engine as it stood before the fused, probe
and projection sites shared one compiler, so instruction streams, registers,
constants, fetch slots and the precomputed per-instruction constants of all
three sites must come out exactly as they did then.
"""
import json

import pytest

from tests.gxlib import load_product
from tools import dump_vm_programs as D

with open(D.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_corpus_is_the_golden_files():
    assert sorted(D.corpus()) == sorted(GOLDEN)
    # all three sites are pinned
    sites = {text.split()[1] for text in GOLDEN.values()}
    assert sites == {"fused", "probe", "projection"}


@pytest.mark.parametrize("name", sorted(D.corpus()))
def test_program_unchanged(name):
    lib = D.declare(load_product())
    assert D.dump(lib, D.corpus()[name]) == GOLDEN[name]


def test_q3_round_leaves_the_probe():
    """ROUND is outside the probe kernel's opcode set: the plan must compile
    to aggregation over joined rows (the fused site), not to the probe."""
    assert GOLDEN["q3"].startswith("site probe ")
    assert GOLDEN["q3_round"].startswith("site fused ")
    assert " op=8 " in GOLDEN["q3_round"]  # VM_ROUND_SCALE


def test_q3_if_keeps_its_operands_on_the_probe():
    """VM_CMP's comparison and VM_IF's else register travel in ins.c."""
    assert GOLDEN["q3_if"].startswith("site probe ")
    cmp_ins = [l for l in GOLDEN["q3_if"].splitlines() if " op=15 " in l]
    if_ins = [l for l in GOLDEN["q3_if"].splitlines() if " op=16 " in l]
    assert len(cmp_ins) == len(if_ins) == 1
    assert " c=2 " in cmp_ins[0]  # GX_F_GT
    assert " c=-1 " not in if_ins[0]
