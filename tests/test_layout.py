"""The layout of tests/ itself: helpers live in modules without tests, and no test file serves as a library.  Parses every
tests/*.py with ast; imports nothing of them."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = sorted(glob.glob(os.path.join(HERE, "*.py")))


def imported_modules(tree):
    """(line, dotted module name) of every import in the tree, function bodies included; `from m import a` also yields m.a, so
    that a test module taken out of a package by name is seen."""
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield node.lineno, a.name
        elif isinstance(node, ast.ImportFrom):
            base = "." * node.level + (node.module or "")
            yield node.lineno, base
            for a in node.names:
                yield node.lineno, f"{base}.{a.name}"


def test_no_test_file_is_imported_and_tests_is_no_package_prefix():
    assert len(FILES) > 40, FILES
    bad = []
    for path in FILES:
        tree = ast.parse(open(path).read(), path)
        for line, name in imported_modules(tree):
            parts = name.split(".")
            # the last component of `from m import a` may be a function: only modules are named test_*.py, functions test_* are
            # never imported either, so both are refused alike
            if parts[-1].startswith("test_") or parts[0] == "tests" or (len(parts) > 1 and parts[-2].startswith("test_")):
                bad.append(f"{os.path.basename(path)}:{line}: {name}")
    assert not bad, bad


def test_only_test_files_define_tests():
    bad = []
    for path in FILES:
        if os.path.basename(path).startswith("test_"):
            continue
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and node.name.startswith("test_"):
                bad.append(f"{os.path.basename(path)}:{node.lineno}: {node.name}")
    assert not bad, bad
