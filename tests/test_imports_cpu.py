"""CPU: no file under tests/ imports from a test module.  What two files share lives in a plain module (gpu_support,
gated_oracle, streams, host_check, the models ...), so that renaming or splitting a test file breaks nothing else."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_no_file_imports_from_a_test_module():
    seen = 0
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if isinstance(node, ast.ImportFrom):
                names = [node.module or ""] + [f"{node.module or ''}.{a.name}" for a in node.names]
            elif isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            else:
                continue
            seen += 1
            for name in names:
                parts = name.lstrip(".").split(".")
                bad = parts[0].startswith("test_") or (parts[0] == "tests" and len(parts) > 1 and parts[1].startswith("test_"))
                assert not bad, f"{os.path.basename(path)}:{node.lineno} imports {name}"
    assert seen > 100                                         # (the walk saw the suite)
