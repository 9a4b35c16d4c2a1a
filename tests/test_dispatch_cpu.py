"""The attention dispatch, pinned: tests/golden/dispatch_census.txt holds a seeded sample of tools/dispatch_census.py's census (which
kernel variant oeh_attn_variant / oeh_attn_variant_ex name for a descriptor, diagnostic hooks at their defaults).  A change of the
dispatch shows up as a reviewed diff of that file:  python tools/dispatch_census.py --golden 1950 > tests/golden/dispatch_census.txt"""
import importlib.util
import os

from tests.conftest import GOLDEN, ROOT


def test_dispatch_census_replays_through_the_c_abi():
    spec = importlib.util.spec_from_file_location("dispatch_census", os.path.join(ROOT, "tools", "dispatch_census.py"))
    census = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(census)
    from outeffhop_amd import _lib

    lib = _lib.load()
    with open(os.path.join(GOLDEN, "dispatch_census.txt")) as f:
        lines = [ln.rstrip("\n") for ln in f if ln.strip()]
    assert len(lines) >= 1900
    assert census.missing_families({ln.split(" | ")[1] for ln in lines}, False) == []  # every kernel family, and "no name"
    census.reset_hooks(lib)  # (another test's hook setting must not leak into the names)
    wrong = []
    for ln in lines:
        case, want = ln.split(" | ")
        got = census.names(lib, census.parse_case(case))
        if got != want:
            wrong.append(f"{case}: {got} (pinned: {want})")
    assert not wrong, f"{len(wrong)} of {len(lines)} cases changed their kernel:\n" + "\n".join(wrong[:20])
