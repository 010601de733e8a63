"""The kernel library's C ABI is written once, in ``csrc/pdt_api.h``: the header, the definitions
in ``csrc/*.hip``, the ctypes table ``ops/native_ops/lib.py`` derives from the header, and the Python
call sites agree. No GPU; only the last test needs the built library."""
import ctypes
import re
from pathlib import Path

import pytest

from pytorch_distributed_template_amd.ops import native_ops as no

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "csrc"
HEADER = (CSRC / "pdt_api.h").read_text()
P, I, L, U, F, D = (ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_uint, ctypes.c_float,
                    ctypes.c_double)


def test_parser_reads_every_declaration_once_within_the_closed_set():
    # parse_api raises on a type outside the closed set and on a name declared twice
    sigs = no.parse_api(HEADER)
    declared = re.findall(r"\bPDT_API\b[^;{]*?\b(pdt_\w+)\s*\(", HEADER)
    assert len(declared) > 100 and len(set(declared)) == len(declared)
    assert list(sigs) == declared
    assert len(re.findall(r"^PDT_API\b", HEADER, re.M)) == len(declared)  # nothing the pattern skipped
    allowed = {P, I, L, U, F, D}
    for name, (res, args) in sigs.items():
        assert res in allowed and set(args) <= allowed, name
    assert no.signatures() == sigs


@pytest.mark.parametrize("decl", [
    "PDT_API int pdt_x(const uint8_t* p);", "PDT_API int pdt_x(long long n);", "PDT_API int pdt_x(int** p);",
    "PDT_API int pdt_x(unsigned int n);", "PDT_API char pdt_x(int n);", "PDT_API int pdt_x(size_t n);"])
def test_type_outside_the_closed_set_raises_and_names_the_declaration(decl):
    with pytest.raises(TypeError, match="pdt_x"):
        no.parse_api(decl)


def test_duplicate_declaration_raises():
    with pytest.raises(ValueError, match="pdt_x"):
        no.parse_api("PDT_API int pdt_x(int n);\nPDT_API int pdt_x(int n);")


def test_declarations_and_definitions_agree():
    defined = []
    for src in sorted(CSRC.glob("*.hip")):
        text = src.read_text()
        # a PDT_API that reaches ';' before '{' is a declaration without a body
        assert not re.findall(r"\bPDT_API\b[^;{]*;", text), f"{src.name}: declare it in pdt_api.h instead"
        defined += re.findall(r"\bPDT_API\b[^;{]*?\b(pdt_\w+)\s*\([^;{]*\{", text)
    assert len(set(defined)) == len(defined)
    assert set(defined) == set(no.signatures())
    for inc in [*CSRC.glob("*.h"), *CSRC.glob("*.inc")]:
        if inc.name != "pdt_api.h":
            assert not re.findall(r"\bPDT_API\s+\w", inc.read_text()), inc.name


def test_every_entry_point_python_reaches_is_declared():
    # every attribute access of a pdt_ name in the package, scripts/, tests/ and bench.py is one on a
    # library handle, except pdt_nhwc_pad (an attribute the loaders set on image tensors)
    files = [*ROOT.glob("pytorch_distributed_template_amd/**/*.py"), *ROOT.glob("scripts/**/*.py"),
             *ROOT.glob("tests/**/*.py"), ROOT / "bench.py"]
    sigs = no.signatures()
    used = {}
    for f in files:
        for name in re.findall(r"\.\s*(pdt_\w+)\b", f.read_text()):
            used.setdefault(name, f.relative_to(ROOT))
    used.pop("pdt_nhwc_pad", None)
    assert len(used) > 100
    assert {n: str(f) for n, f in used.items() if n not in sigs} == {}


def test_four_signatures_literally():
    sigs = no.signatures()
    assert sigs["pdt_conv_nt"] == (I, [P] * 7 + [I] * 25 + [P, I, I, P])
    assert sigs["pdt_bn_finalize"] == (I, [P, I, I, D, F, F] + [P] * 9 + [P])
    assert sigs["pdt_fill_uniform_bf16"] == (I, [P, L, U, P])
    assert sigs["pdt_wgrad_workspace"] == (L, [I, I, I])


def test_load_binds_every_declared_name():
    if not no.lib_path().exists():
        pytest.skip("kernel library not built")
    lib = no._load()
    lib = getattr(lib, "_lib", lib)  # under PDT_OP_TIMING the handle is wrapped
    for name, (res, args) in no.signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
