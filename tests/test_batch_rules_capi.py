"""CPU: the C ABI of a batch's per-board rules (gol_rules_batch_*; DESIGN.md
section 5k).  No device is touched: the symbols, their declarations and the
binding's prototypes, the rule word in C and in Python, and what
gol_rules_batch_check accepts and refuses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import batch_rules_model as RM
from gameoflife import _native as N
from gameoflife import batch, rules
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = ("gol_rules_batch_check", "gol_rules_batch_set", "gol_rules_batch_get")
_P = ctypes.POINTER
CTYPES = {"gol_batch*": ctypes.c_void_p, "constgol_batch_config*": _P(N.GolBatchConfig), "int64_t": ctypes.c_int64,
          "uint32_t*": _P(ctypes.c_uint32), "constuint32_t*": _P(ctypes.c_uint32)}
FOUR = ("life", "ref-literal", "ref-effective", "B36/S23")


def _declaration(name):
    """Parameter types of `name` as include/gol.h declares it."""
    text = open(N.HEADER_PATH).read()
    m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, text, re.M)
    assert m, f"include/gol.h does not declare int {name}(...)"
    return ["".join(p.replace("*", "* ").split()[:-1]) for p in m.group(1).split(",")]


def _cfg(boards=3, width=8, height=8, topology=N.GOL_TORUS):
    c = N.GolBatchConfig()
    c.boards, c.width, c.height, c.topology = boards, width, height, topology
    c.birth_mask, c.survive_mask = O.LIFE
    return c


def _check(cfg, first, count, words):
    ptr = None
    if words is not None:
        words = np.ascontiguousarray(words, dtype=np.uint32)
        ptr = words.ctypes.data_as(N._u32p)
    return N.lib.gol_rules_batch_check(ctypes.byref(cfg), first, count, ptr)


def _error():
    return N.lib.gol_batch_last_error(None).decode()


def test_declared_exported_and_bound():
    syms = N.header_symbols()
    for name in RULES:
        assert name in syms, name
        assert hasattr(N.lib, name), name
        assert name in N._SIGNATURES, name
    assert sorted(s for s in syms if s.startswith("gol_rules_batch")) == sorted(RULES)


def test_prototypes_match_header():
    for name in RULES:
        res, args = N._SIGNATURES[name]
        assert res is ctypes.c_int and args == [CTYPES[t] for t in _declaration(name)], name
        fn = getattr(N.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert _declaration("gol_rules_batch_set") == ["gol_batch*", "int64_t", "int64_t", "constuint32_t*"]
    assert _declaration("gol_rules_batch_get") == ["gol_batch*", "int64_t", "int64_t", "uint32_t*"]
    assert _declaration("gol_rules_batch_check") == ["constgol_batch_config*", "int64_t", "int64_t", "constuint32_t*"]
    assert N.lib.gol_abi_version() == 2


def test_rule_word_round_trips():
    for name in FOUR:
        r = rules.rule_by_name(name)
        w = rules.rule_word(name)
        assert w == rules.rule_word(r) == rules.rule_word((r.birth, r.survive)) == r.birth | (r.survive << 16)
        back = rules.rule_from_word(w)
        assert (back.birth, back.survive) == (r.birth, r.survive)
        assert rules.rule_word(back) == w
        assert back.name == (name if name in rules.NAMED else r.notation())
    assert rules.rule_word("life") == 0x000C0008
    assert rules.rule_from_word(0x000C0048).notation() == "B36/S23"
    for bad in (1 << 9, 1 << 25, 1 << 31):
        with pytest.raises(ValueError):
            rules.rule_from_word(bad)
    with pytest.raises(ValueError):
        rules.rule_word((0x200, 0))


def test_macro_agrees_with_rule_word(tmp_path):
    pairs = [(r.birth, r.survive) for r in map(rules.rule_by_name, FOUR)] + [(0, 0), (0x1FF, 0x1FF), (0x155, 0x0AA)]
    src = tmp_path / "w.c"
    src.write_text('#include <stdio.h>\n#include "gol.h"\nint main(void){\n'
                   + "".join(f'printf("%u ", GOL_BATCH_RULE({b}, {s}));\n' for b, s in pairs) + "return 0;}\n")
    exe = tmp_path / "w"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [rules.rule_word(p) for p in pairs]
    assert all(w & ~N.GOL_BATCH_RULE_BITS == 0 for w in got)


def test_rule_sweep_words():
    w = batch.rule_sweep_words([0x008, 0x048], [0x00C, 0x1FF, 0])
    assert w.dtype == np.uint32
    assert w.tolist() == [rules.rule_word((b, s)) for b in (0x008, 0x048) for s in (0x00C, 0x1FF, 0)]
    with pytest.raises(ValueError):
        batch.rule_sweep_words([0x200], [0])
    with pytest.raises(ValueError):
        batch.rule_sweep_words([0], [-1])


def test_check_accepts_every_life_like_rule():
    words = batch.rule_sweep_words(range(512), range(512))
    assert words.size == 1 << 18 and np.unique(words).size == 1 << 18
    assert int(np.bitwise_or.reduce(words)) == 0x01FF01FF
    assert _check(_cfg(boards=1 << 18), 0, 1 << 18, words) == N.GOL_OK
    # ... and a part of them on a part of a batch, and NULL for the whole batch
    assert _check(_cfg(boards=1 << 18), (1 << 18) - 5, 5, words[:5]) == N.GOL_OK
    assert _check(_cfg(boards=1 << 22, width=64, height=64), (1 << 22) - 1, 1, words[-1:]) == N.GOL_OK
    assert _check(_cfg(), 0, 3, None) == N.GOL_OK
    assert _check(_cfg(boards=40), 0, 40, RM.rule_words(40)) == N.GOL_OK


@pytest.mark.parametrize("bit", [9, 25, 15, 26, 31])
def test_check_refuses_a_bad_word_and_names_its_index(bit):
    words = RM.rule_words(40)
    words[23] |= np.uint32(1 << bit)
    assert _check(_cfg(boards=40), 0, 40, words) == N.GOL_EINVAL
    assert "rules[23]" in _error() and "board 23" in _error(), _error()
    assert f"0x{int(words[23]):08X}" in _error()
    # the index is the word's, the board follows from first
    assert _check(_cfg(boards=40), 10, 30, words[10:]) == N.GOL_EINVAL
    assert "rules[13]" in _error() and "board 23" in _error(), _error()
    # the first bad word is the one named
    words[31] |= np.uint32(1 << bit)
    assert _check(_cfg(boards=40), 0, 40, words) == N.GOL_EINVAL
    assert "rules[23]" in _error() and "rules[31]" not in _error()


def test_check_refuses_bad_ranges():
    words = RM.rule_words(8)
    refusals = {
        "first -1": (-1, 1), "count 0": (0, 0), "count -1": (0, -1), "first = boards": (3, 1),
        "past the end": (1, 3), "count 2^62": (1, 1 << 62),
    }
    for what, (first, count) in refusals.items():
        assert _check(_cfg(), first, count, words) == N.GOL_EINVAL, what
        assert "outside the batch" in _error(), (what, _error())


def test_check_refuses_null_rules_for_a_part():
    for first, count in ((0, 2), (1, 2), (2, 1)):
        assert _check(_cfg(), first, count, None) == N.GOL_EINVAL
        assert "rules is null" in _error()
    assert N.lib.gol_rules_batch_check(None, 0, 1, None) == N.GOL_EINVAL
    # a geometry gol_batch_create refuses is refused here alike
    assert _check(_cfg(width=65), 0, 3, RM.rule_words(3)) == N.GOL_EINVAL
    assert _check(_cfg(width=2), 0, 3, RM.rule_words(3)) == N.GOL_EINVAL


def test_null_handle_is_einval_and_writes_nothing():
    words = np.full(4, 0xDEAD, dtype=np.uint32)
    assert N.lib.gol_rules_batch_set(None, 0, 4, words.ctypes.data_as(N._u32p)) == N.GOL_EINVAL
    assert N.lib.gol_rules_batch_get(None, 0, 4, words.ctypes.data_as(N._u32p)) == N.GOL_EINVAL
    assert _error() and (words == 0xDEAD).all()


def test_model_rule_list():
    w = RM.rule_words(40)
    assert w[:7].tolist() == [rules.rule_word(n) for n in RM.NAMED]
    assert RM.masks(w[2])[0] & 1  # a birth on 0 neighbours is among them
    assert all(int(x) & ~0x01FF01FF == 0 for x in w) and np.unique(w[7:]).size == 33
    assert RM.named_words(15).tolist() == (w[:7].tolist() * 3)[:15]


def test_python_wrapper_has_the_calls():
    assert callable(batch.GolBatch.set_rules) and callable(batch.GolBatch.rules) and callable(batch.rule_sweep_words)
