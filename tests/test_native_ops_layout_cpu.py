"""``ops/native_ops/`` is a package of one module per kernel family behind a facade that re-exports
every name: each name the rest of the tree reaches through the facade is there, and the modules
import each other's names in one direction only. No GPU and no built library."""
import ast
import re
from pathlib import Path

from pytorch_distributed_template_amd.ops import native_ops

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "pytorch_distributed_template_amd" / "ops" / "native_ops"
MODULES = {f.stem: ast.parse(f.read_text()) for f in sorted(PKG.glob("*.py")) if f.stem != "__init__"}


def test_every_name_reached_through_the_facade_is_reexported():
    # ``native_ops.NAME`` anywhere, ``no.NAME`` where the file imports the package under that alias,
    # and the names of ``from ...native_ops[.module] import NAME[, NAME]`` statements -- those the
    # package's own modules import from each other (``from .module import NAME``) included
    files = [*ROOT.glob("pytorch_distributed_template_amd/**/*.py"), *ROOT.glob("scripts/**/*.py"),
             *ROOT.glob("tests/**/*.py"), ROOT / "bench.py"]
    used = {}
    for f in files:
        if f == Path(__file__).resolve():
            continue
        text = f.read_text()
        names = re.findall(r"\bnative_ops\.([A-Za-z_]\w*)", text)
        if re.search(r"\bnative_ops as no\b", text):
            names += re.findall(r"\bno\.([A-Za-z_]\w*)", text)
        source = r"[\w.]*\bnative_ops(?:\.\w+)?" + (r"|\.\w+" if f.parent == PKG else "")
        for stmt in re.findall(rf"^\s*from\s+(?:{source})\s+import\s+(\([^)]*\)|[^\n#]+)", text, re.M):
            names += [n.split(" as ")[0].strip() for n in stmt.strip("() \t").split(",") if n.strip()]
        for name in names:
            used.setdefault(name, f.relative_to(ROOT))
    assert len(used) > 100
    # each pattern found what the tree is known to reach that way (bench.py and the trainer import
    # names, ops/fused.py goes through ``native_ops.``, the tests through ``no.``)
    assert {"fp8_settings", "nhwc_padded_view", "check_targets_pending", "available", "_load", "_p", "_s", "_chk",
            "_nt_args", "_ax_launch", "_BNArgs", "_unit_fwd_s2d", "_conv_dgrad", "_SHADOWS", "_FALLBACK_WARNED",
            "_LIB_PATH"} <= set(used)
    assert {n: str(f) for n, f in used.items() if not hasattr(native_ops, n)} == {}


def _intra_package_imports(tree):
    """Modules of this package that ``tree`` imports names from, at any depth of the code."""
    deps = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level == 1:
            assert node.module is not None, "import the names from their module, not a module from the facade"
            deps.add(node.module.split(".")[0])
        elif isinstance(node, ast.ImportFrom):
            assert "native_ops" not in (node.module or "").split("."), "a module imports the facade"
            assert node.level != 2 or "native_ops" not in [a.name for a in node.names], "a module imports the facade"
        elif isinstance(node, ast.Import):
            assert not any("native_ops" in a.name.split(".") for a in node.names), "a module imports the facade"
    return deps


def test_modules_import_each_other_in_one_direction_and_the_facade_defines_nothing():
    graph = {name: _intra_package_imports(tree) for name, tree in MODULES.items()}
    assert len(graph) > 10 and all(deps <= set(graph) for deps in graph.values()), graph
    done = set()
    while len(done) < len(graph):  # peel off modules whose imports are all peeled: a cycle stops it
        ready = {m for m, deps in graph.items() if m not in done and deps <= done}
        assert ready, f"import cycle among {sorted(set(graph) - done)}"
        done |= ready
    facade = ast.parse((PKG / "__init__.py").read_text())
    assert not [n for n in ast.walk(facade) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef,
                                                              ast.Lambda))]
    for name, tree in MODULES.items():  # and every public or private name of every module is on the facade
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                assert getattr(native_ops, node.name) is getattr(__import__(
                    f"{native_ops.__name__}.{name}", fromlist=[node.name]), node.name), (name, node.name)
