"""CPU: the committed csrc/deform_mlp16_kloop.inc is what tools/gen_mlp16_kloop.py writes, and its macros are exactly the ones
csrc/deform_mlp16.hip uses.  The GPU test of these statements (test_gpu_deform.py: bit identity with the compiler-scheduled loops)
never looks at the generator, so an edit to one of the two without the other would otherwise go unnoticed."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "gen_mlp16_kloop.py")
CSRC = os.path.join(ROOT, "gaussianprediction_amd", "csrc")

_spec = importlib.util.spec_from_file_location("gen_mlp16_kloop", GEN)
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
RENDERED = gen.render()


def _read(name):
    with open(os.path.join(CSRC, name), newline="") as f:
        return f.read()


def test_the_committed_inc_is_what_the_generator_writes():
    committed = _read("deform_mlp16_kloop.inc")
    if committed != RENDERED:
        a, b = committed.split("\n"), RENDERED.split("\n")
        n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError(
            f"deform_mlp16_kloop.inc differs from the generator's text, first at line {n + 1}:\n"
            f"  committed: {a[n] if n < len(a) else '<end of file>'}\n  generated: {b[n] if n < len(b) else '<end of file>'}\n"
            "regenerate it with: python tools/gen_mlp16_kloop.py")


def test_the_generator_defines_exactly_the_macros_the_kernels_use():
    # name -> body (a definition ends at the first line without a trailing backslash)
    defs = {m.group(1): m.group(2) for m in re.finditer(r"^#define (\w+)((?:.*\\\n)*.*)$", RENDERED, re.M)}
    assert len(defs) == len(re.findall(r"^#define ", RENDERED, re.M)), "a macro is defined twice"
    used = set(re.findall(r"\bM16[SP]_\w+_(?:ASM|CLOBBERS)\b", _read("deform_mlp16.hip")))
    assert used, "deform_mlp16.hip uses none of the generated macros"
    assert used <= set(defs), f"used in deform_mlp16.hip, not defined by the generator: {sorted(used - set(defs))}"
    reached, todo = set(), sorted(used)
    while todo:
        name = todo.pop()
        if name not in reached:
            reached.add(name)
            todo += [w for w in re.findall(r"\b\w+\b", defs[name]) if w in defs]
    assert reached == set(defs), f"defined by the generator, used nowhere: {sorted(set(defs) - reached)}"


def test_rendering_twice_gives_the_same_text():
    assert gen.render() == RENDERED
