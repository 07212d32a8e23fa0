"""The two bindings have one surface: every operator of the TORCH_LIBRARY(newt_hip) block of csrc/torch_ops.cpp has a
`_cops.CtypesOps` method of the same name with the same positional parameters, and the other way round.  `engine.binding()`
hands out one or the other, so a call site written against the op schema must be a valid call of the ctypes object too.
Text and signatures only: no GPU, no library load."""
import importlib
import inspect
import os
import re

from conftest import ROOT

PKG = "neural-waveshaping-synthesis_amd"


def op_schemas():
    """{op name: [parameter names in order]} from the m.def("name(args) -> ret", ...) lines of the TORCH_LIBRARY block"""
    with open(os.path.join(ROOT, PKG, "csrc", "torch_ops.cpp")) as f:
        text = f.read()
    block = text[text.index("TORCH_LIBRARY(newt_hip"):]
    schemas = {}
    for m in re.finditer(r'm\.def\(\s*((?:"[^"]*"\s*)+),', block):       # a schema may be split over adjacent string literals
        schema = "".join(re.findall(r'"([^"]*)"', m.group(1)))
        name, args, _ = re.fullmatch(r"(\w+)\((.*)\)\s*->\s*(.+)", schema).groups()
        assert name not in schemas, name
        schemas[name] = [a.split()[-1] for a in args.split(",") if a.strip()]      # "Tensor(a!)? pre_out" -> "pre_out"
    assert block.count("m.def(") == len(schemas)          # every m.def of the block was understood
    return schemas


def test_ctypes_object_mirrors_every_op_schema():
    schemas = op_schemas()
    assert len(schemas) >= 30 and {"forward", "stream_step_slots", "g_gru", "loudness", "abi_version"} <= set(schemas)
    cops = importlib.import_module(PKG + "._cops").CtypesOps
    for name, params in schemas.items():
        fn = inspect.getattr_static(cops, name, None)
        assert inspect.isfunction(fn), f"CtypesOps has no method for the op {name}"
        sig = list(inspect.signature(fn).parameters.values())
        assert sig[0].name == "self", name
        assert all(p.kind is p.POSITIONAL_OR_KEYWORD and p.default is p.empty for p in sig), name
        assert [p.name for p in sig[1:]] == params, f"{name}: op schema {params}, CtypesOps {[p.name for p in sig[1:]]}"


def test_ctypes_object_has_no_method_without_an_op():
    schemas = op_schemas()
    cops = importlib.import_module(PKG + "._cops").CtypesOps
    public = {n for n, v in vars(cops).items() if not n.startswith("_") and callable(v)}
    assert public == set(schemas), public ^ set(schemas)
