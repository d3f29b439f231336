"""Test modules are no library for each other: no file under tests/, tests/golden/ or tools/ imports a module whose name starts with test_.  What two test
modules share lives in a support module (helpers.py, a *_cases.py, a *_twin.py, bench_slice.py), where pytest does not collect it and an edit is an edit to
shared code in plain sight."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sources():
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "golden", "*.py"))
    files += glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True)
    return sorted(files)


def _imported_modules(node):
    """the dotted module names an import statement names, anywhere in a file (ast.walk reaches function bodies)"""
    if isinstance(node, ast.Import):
        return [a.name for a in node.names]
    if isinstance(node, ast.ImportFrom):
        base = node.module or ""
        return [base] + [f"{base}.{a.name}" if base else a.name for a in node.names]      # a name taken out of a package may be a module too
    return []


def test_no_module_imports_a_test_module():
    files = _sources()
    assert len(files) > 90 and any(f.endswith(os.path.join("tools", "experiments", "sharded_ladder_diag.py")) for f in files), len(files)
    bad = []
    for path in files:
        tree = ast.parse(open(path, encoding="utf-8").read(), filename=path)
        for node in ast.walk(tree):
            for name in _imported_modules(node):
                if any(part.startswith("test_") for part in name.split(".")):
                    bad.append(f"{os.path.relpath(path, ROOT)}:{node.lineno}: imports {name}")
    assert not bad, "test modules imported as libraries (move what is shared into a support module):\n" + "\n".join(bad)
