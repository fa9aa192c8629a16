"""Build-container script (needs the reference tree; NOT run on the GPU box): walks the two reference files that reach
`kmeans_pytorch` and `torch_scatter` with `ast`, with the walker of make_extension_surface.py, and records every import of and call
into them: the dotted callee, the number of positional arguments, the keyword names, the arity of the tuple the call site unpacks
(null where it does not unpack) and file:line.  A call through a local that a function binds over an imported name is left out.  Writes tests/golden/kmeans_surface.json (data: names and counts);
tests/test_kmeans_host.py binds every recorded call to this repository's shims.

    python tests/golden/make_kmeans_surface.py [/path/to/reference]
"""
import ast
import json
import os

import make_extension_surface as S

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kmeans_surface.json")
S.FILES = ["utils/visualizer_utils.py", "scene/gaussian_model.py"]
S.MODULES = ("kmeans_pytorch", "torch_scatter")


def _rebound(tree):
    """{function: names it stores to}: `cluster` binds a local `kmeans` (an sklearn estimator) over the imported function, and a
    call through that local is no call into the module."""
    return {f.name: {n.id for n in ast.walk(f) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store)}
            for f in ast.walk(tree) if isinstance(f, ast.FunctionDef)}


def main():
    out = {"_generated_by": "tests/golden/make_kmeans_surface.py (ast walk; names and counts only)", "imports": [], "calls": []}
    global_alias, parsed = {}, []
    for rel in S.FILES:
        tree, alias, imports, calls = S.walk(rel, global_alias)
        out["imports"] += imports
        parsed.append((rel, tree, alias, calls))
    for rel, tree, alias, calls in parsed:
        S.walk_calls(rel, tree, alias, {}, calls)     # (a bare name resolves through the file's own imports only)
        local = _rebound(tree)
        heads = {v: k for k, v in alias.items()}
        calls = [c for c in calls if not any(c["callee"].startswith(full) and name in local.get(c["in"], ()) for full, name in heads.items())]
        out["calls"] += sorted(calls, key=lambda c: int(c["where"].rsplit(":", 1)[1]))
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(out['imports'])} imports, {len(out['calls'])} calls")


if __name__ == "__main__":
    main()
