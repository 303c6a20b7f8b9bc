"""ingress::k_update_members<R> (bk_update_members) is in the shipped library for every pool size, compiles to the
instruction counts and loop sizes of profiles/kernel_isa_members_ingress.json within the baseline's 3 %, and uses no scratch
memory; and the set of kernels tools/kernel_isa_counts.py::measure names - the shipped set of
profiles/kernel_isa_baseline.json, which tests/kernel_cases.py covers case by case - is exactly what it was: the new kernel
sits in a nested namespace and is covered here and by tests/members_ingress_cases.py instead."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _lib():
    import kernel_isa_counts as K
    from bourse_amd import _build

    if not all(K._tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")):
        pytest.skip("no llvm-objdump / clang-offload-bundler")
    return _build.build()  # (rebuilds when a source is newer than the library: the counts are of THIS tree's code)


def test_every_instantiation_is_shipped_matches_its_profile_and_uses_no_scratch():
    import kernel_isa_counts as K
    import members_ingress_isa as M

    dis = M.disassemble(_lib())
    assert sorted(dis) == [f"ingress::k_update_members<{R}>" for R in (1, 2, 4, 8)]
    base = json.load(open(M.PROFILE))
    assert base["_tolerance"] == json.load(open(K.BASELINE))["_tolerance"] == K.TOL
    bad = K.compare(base["kernels"], {k: v for k, (v, _) in dis.items()}, base["_tolerance"])
    assert not bad, ("instruction counts moved by more than 3 % against profiles/kernel_isa_members_ingress.json (profile "
                     f"toolchain: {base['_toolchain']}; now: {K.toolchain()}).  If the change is intended: "
                     "python tools/members_ingress_isa.py --update.\n" + "\n".join(bad[:40]))
    for name, (v, ops) in dis.items():
        assert v["counts"]["total"] == len(ops) > 1000, name
        assert not [op for op in ops if op.startswith("scratch_")], name
        assert not [op for op in ops if op.startswith("ds_")], (name, "the kernel keeps no table in LDS")
        assert v["loops"], name


def test_the_shipped_set_of_the_baseline_is_unchanged():
    import kernel_isa_counts as K

    now = K.measure(_lib())
    base = json.load(open(K.BASELINE))["kernels"]
    assert sorted(now) == sorted(base)
    assert not [k for k in now if "k_update_members" in k]
