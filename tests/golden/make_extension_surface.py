"""Build-container script (needs the reference tree; NOT run on the GPU box): walks the reference files that reach the CUDA-only
extension modules with `ast` and records, for every import of and call into them, the dotted callee, the number of positional
arguments, the keyword names, the arity of the tuple the call site unpacks (null where it does not unpack) and file:line.  Writes
tests/golden/extension_surface.json (data: names and counts); tests/test_extension_shims.py binds every recorded call to this
repository's shims.

    python tests/golden/make_extension_surface.py [/path/to/reference]
"""
import ast
import json
import os
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "extension_surface.json")
FILES = ["scene/gaussian_model.py", "utils/fps.py", "utils/loss_utils.py", "utils/camera_utils.py"]
MODULES = ("simple_knn._C", "tinycudann", "pytorch3d.ops", "pytorch3d.transforms", "frnn", "pointops_cuda")


def _ours(dotted):
    return any(dotted == m or dotted.startswith(m + ".") for m in MODULES)


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if not isinstance(node, ast.Name):
        return None
    parts.append(node.id)
    return ".".join(reversed(parts))


def walk(rel, global_alias):
    """imports and calls of one file.  A bare name that the file uses without importing it (utils/loss_utils.py calls knn_points
    with no import of its own) resolves through the other files' imports and is recorded with "imported_here": false."""
    tree = ast.parse(open(os.path.join(REF, rel)).read())
    alias, imports, calls = {}, [], []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                if _ours(a.name):
                    alias[a.asname or a.name] = a.name
                    imports.append({"import": a.name, "as": a.asname, "where": f"{rel}:{node.lineno}"})
        elif isinstance(node, ast.ImportFrom) and node.module and _ours(node.module):
            for a in node.names:
                alias[a.asname or a.name] = f"{node.module}.{a.name}"
                imports.append({"import": f"{node.module}.{a.name}", "as": a.asname, "where": f"{rel}:{node.lineno}"})
    global_alias.update(alias)
    return tree, alias, imports, calls


def walk_calls(rel, tree, alias, global_alias, calls):
    enclosing = {}
    for top in ast.walk(tree):
        if isinstance(top, (ast.FunctionDef, ast.ClassDef)):
            for child in ast.walk(top):
                if isinstance(child, ast.Call) and (id(child) not in enclosing or isinstance(top, ast.FunctionDef)):
                    enclosing[id(child)] = top.name
    unpacked = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Call) and len(node.targets) == 1 \
                and isinstance(node.targets[0], ast.Tuple):
            unpacked[id(node.value)] = len(node.targets[0].elts)
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        name = _dotted(node.func)
        if name is None:
            continue
        head, _, rest = name.partition(".")
        table = alias if head in alias else global_alias
        if head not in table:
            continue
        callee = table[head] + ("." + rest if rest else "")
        calls.append({"callee": callee, "positional": len(node.args), "keywords": [k.arg for k in node.keywords],
                      "unpacked": unpacked.get(id(node)), "imported_here": head in alias, "in": enclosing.get(id(node)),
                      "where": f"{rel}:{node.lineno}"})


def main():
    out = {"_generated_by": "tests/golden/make_extension_surface.py (ast walk; names and counts only)", "imports": [], "calls": []}
    global_alias, parsed = {}, []
    for rel in FILES:
        tree, alias, imports, calls = walk(rel, global_alias)
        out["imports"] += imports
        parsed.append((rel, tree, alias, calls))
    for rel, tree, alias, calls in parsed:
        walk_calls(rel, tree, alias, global_alias, calls)
        out["calls"] += sorted(calls, key=lambda c: int(c["where"].rsplit(":", 1)[1]))
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(out['imports'])} imports, {len(out['calls'])} calls")


if __name__ == "__main__":
    main()
