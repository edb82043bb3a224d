"""The inventory of kernel C's instances and pack groups (CPU): every distinct POA_VARIANT of poa.hip's tables and every group kind of
poa_device_run is named in tests/test_gpu_poa_variants.py together with the GPU case that compares it with the oracle.  A variant added to
a table, or a case dropped from the list, fails here."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POA = os.path.join(ROOT, "rattle_amd", "csrc", "poa.hip")
GPU_MODULE = os.path.join(ROOT, "tests", "test_gpu_poa_variants.py")


def _source():
    with open(POA) as f:
        return f.read()


def _defines(src):
    return {m[1]: int(m[2]) for m in re.finditer(r"^#define (\w+) (\d+)\b", src, re.M)}


def _module_dicts():
    """VARIANTS, GROUPS and the test functions of the GPU module, read without importing it"""
    tree = ast.parse(open(GPU_MODULE).read())
    out, funcs = {}, set()
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and getattr(node.targets[0], "id", None) in ("VARIANTS", "GROUPS"):
            out[node.targets[0].id] = ast.literal_eval(node.value)
        if isinstance(node, ast.FunctionDef) and node.name.startswith("test_"):
            funcs.add(node.name)
    return out["VARIANTS"], out["GROUPS"], funcs


def _table_variants(src):
    """the template arguments of every POA_VARIANT(...) in the variant tables, the macros resolved, duplicates removed"""
    d = _defines(src)
    start = src.index("#define POA_VARIANT(")
    end = src.index("struct poa_env")
    found = set()
    for args in re.findall(r"POA_VARIANT\(([^()]*)\)", src[src.index("\n", start):end]):
        toks = [t.strip() for t in args.split(",")]
        assert len(toks) == 4, args
        found.add(tuple(int(t) if t.isdigit() else d[t] for t in toks))
    return found


def test_every_variant_has_a_gpu_case():
    variants, _, funcs = _module_dicts()
    found = _table_variants(_source())
    assert len(found) >= 26
    assert set(variants) == found, (sorted(found - set(variants)), sorted(set(variants) - found))
    for v, case in variants.items():
        assert case.split("[")[0] in funcs, (v, case)


def test_every_group_kind_has_a_gpu_case():
    src = _source()
    d = _defines(src)
    _, groups, funcs = _module_dicts()
    assert sorted(groups) == list(range(d["POA_GROUPS"]))
    for g, case in groups.items():
        assert case.split("[")[0] in funcs, (g, case)
    # the restatement of the group helpers the GPU module's comments and _group_of rely on, checked against the source
    assert "static inline int poa_group_class(int g) { return g < POA_CLASSES ? g : g < 12 ? g - 4 : g < 16 ? g - 12 : g < 20 ? g - 16 : g - 20; }" in src
    assert "static inline bool poa_group_chain(int g) { return (g >= 12 && g < 16) || g >= 20; }" in src
    assert "static inline bool poa_group_band(int g) { return g >= 16; }" in src
    assert "if (cls >= 4 && pack_first[p + 1] - pack_first[p] <= POA_SHALLOW_READS) cls += 4;" in src
    assert "if (cls < 4 && pack_first[p + 1] - pack_first[p] > POA_CHAIN_SEQS) cls += 12;" in src
    assert "if (band_pack) cls += cls >= 12 ? 8 : 16;" in src
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_poa_variants as m
    assert (m.POA_CHAIN_SEQS, m.POA_BAND_SPREAD, m.POA_SHALLOW_READS) == (d["POA_CHAIN_SEQS"], d["POA_BAND_SPREAD"], d["POA_SHALLOW_READS"])
    assert "static const uint32_t k_class_cols[POA_CLASSES - 1] = {%s};" % ", ".join(map(str, m.CLASS_COLS)) in src
