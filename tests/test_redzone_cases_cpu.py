"""tests/redzone_cases.py held to the files it speaks about: the test files (parsed, not imported), the signature table of
bootstrapper_amd/_lib.py and the prototypes of include/bsmi.h and include/bsmi_io.h (read as text)."""
import ast
import glob
import os
import re

import redzone_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _test_functions(path):
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def _table():
    src = open(os.path.join(ROOT, "bootstrapper_amd", "_lib.py")).read()
    body = src[src.index("sigs = {"):src.index("for name, (res, args) in sigs.items()")]
    names = re.findall(r'^\s*"(bsmi_\w+)":\s*\(', body, flags=re.M)
    assert len(names) > 100 and len(names) == len(set(names))
    return set(names)


def _prototypes():
    """entry point -> parameter names, of include/bsmi.h and include/bsmi_io.h"""
    src = open(os.path.join(ROOT, "include", "bsmi.h")).read() + open(os.path.join(ROOT, "include", "bsmi_io.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    protos = {}
    for m in re.finditer(r"\b(bsmi_\w+)\s*\(([^;{}()]*)\)\s*;", src):
        params = [re.sub(r"\[[^\]]*\]", "", p).strip() for p in m.group(2).split(",")]
        protos[m.group(1)] = [re.split(r"[\s*]+", p)[-1] for p in params if p and p != "void"]
    assert len(protos) > 100
    return protos


def test_every_node_id_names_a_test_that_exists():
    assert RC.FAMILIES and all(RC.FAMILIES.values())
    for family, ids in RC.FAMILIES.items():
        assert len(ids) == len(set(ids)), family
        for node in ids:
            path, _, rest = node.partition("::")
            assert re.fullmatch(r"tests/test_\w+_gpu\.py", path) and os.path.exists(os.path.join(ROOT, path)), node
            name = rest.split("[")[0]
            assert name in _test_functions(path), f"{family}: {node} names no test function of {path}"


def test_files_with_nothing_left_out_are_listed_whole():
    listed = {}
    for ids in RC.FAMILIES.values():
        for node in ids:
            path, _, rest = node.partition("::")
            listed.setdefault(path, set()).add(rest.split("[")[0])   # every function; its parameter sets may be thinned
    for path in RC.WHOLE:
        assert listed.get(path) == _test_functions(path), f"{path}: {sorted(_test_functions(path) ^ listed.get(path, set()))}"


def test_excluded_entry_points_are_in_the_table_and_have_a_reason():
    table = _table()
    for name, reason in RC.EXCLUDED.items():
        assert name in table, f"{name} is not in the signature table of bootstrapper_amd/_lib.py"
        assert isinstance(reason, str) and reason.strip(), name


def test_no_entry_point_with_a_device_pointer_is_excluded_without_a_need():
    protos = _prototypes()
    assert "affs_dev" in protos["bsmi_ws_fragments_u8"] and not any(p.endswith("_dev") for p in protos["bsmi_mws_cluster"])
    assert "frames_dev" in protos["bsmi_blosc_encode_dev_u8"]
    assert not _table() - set(protos), f"in the signature table without a prototype: {sorted(_table() - set(protos))}"
    for name, reason in RC.EXCLUDED.items():
        dev = [p for p in protos[name] if p.endswith("_dev")]
        if dev:
            assert reason.startswith("needs:") and len(reason) > len("needs:") + 10, f"{name} takes {dev}: {reason!r}"


def test_every_gpu_test_file_is_used_or_named():
    files = {os.path.relpath(p, ROOT).replace(os.sep, "/") for p in glob.glob(os.path.join(ROOT, "tests", "test_*_gpu.py"))}
    used = {node.partition("::")[0] for ids in RC.FAMILIES.values() for node in ids}
    assert used <= files and set(RC.NOT_USED) <= files
    assert not used & set(RC.NOT_USED), sorted(used & set(RC.NOT_USED))
    assert all(isinstance(r, str) and r.strip() for r in RC.NOT_USED.values())
    unaccounted = sorted(files - used - set(RC.NOT_USED))
    assert not unaccounted, f"neither in a family nor in NOT_USED of tests/redzone_cases.py: {unaccounted}"
