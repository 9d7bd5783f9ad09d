"""Names of the statistics the reference's workflows configure, recorded as data for xdem_amd.stats (needs the reference source
tree, so it runs only where that tree is present; the fixture it writes is what the tests read).

Read from the reference's source text, without importing it (its package needs geoutils):
  * ``STATS_METHODS``   xdem/workflows/schemas.py: the configuration vocabulary of ``DEM.get_stats``;
  * ``_ALIAS``          xdem/workflows/workflows.py: those names -> the labels of the reports.
Written to tests/golden/stats_names.json; names only, no program text.

    python tools/gen_golden_stats.py
"""
from __future__ import annotations

import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from _refimport import REFERENCE_ROOT  # noqa: E402


def literal(path: str, name: str):
    """The literal assigned to the module-level `name` in the file at `path`."""
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return ast.literal_eval(node.value)
    raise RuntimeError(f"{name} not found in {path}")


def main() -> None:
    wf = os.path.join(REFERENCE_ROOT, "xdem", "workflows")
    methods = literal(os.path.join(wf, "schemas.py"), "STATS_METHODS")
    alias = literal(os.path.join(wf, "workflows.py"), "_ALIAS")
    assert all(isinstance(m, str) for m in methods) and all(isinstance(k, str) and isinstance(v, str) for k, v in alias.items())
    out = os.path.join(ROOT, "tests", "golden", "stats_names.json")
    with open(out, "w") as f:
        json.dump({"STATS_METHODS": methods, "_ALIAS": alias}, f, indent=1)
        f.write("\n")
    print(f"wrote {out}: {len(methods)} names, {len(alias)} aliases")


if __name__ == "__main__":
    main()
