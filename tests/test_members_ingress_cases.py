"""The case table of ingress::k_update_members (tests/members_ingress_cases.py) names every instantiation of
profiles/kernel_isa_members_ingress.json, and nothing else, with a well-formed and reachable configuration: an instantiation
without a GPU parity case fails here, on the CPU.  tests/test_gpu_members_with_ingress.py parametrises over the table."""
import subprocess
import sys

import members_ingress_cases as M


def test_the_table_names_exactly_the_profiled_instantiations():
    assert set(M.CASES) == M.profile_kernels()
    assert sorted(M.CASES) == [f"{M.FAMILY}<{R}>" for R in (1, 2, 4, 8)]


def test_every_entry_is_well_formed_and_reachable():
    for name, c in M.CASES.items():
        assert c["name"] == name and name == f"{M.FAMILY}<{c['R']}>"
        assert c["unreachable"] is None, (name, "every instantiation is reachable from the public API")
        assert c["pool"] == 64 * c["R"] == M.POOLS[c["R"]], name  # bk_update_members launches R = max_live_orders / 64
        assert c["books"] >= 64 and c["steps"] >= 30, name
        assert tuple(c["sets"]) == M.SETS, name
        for which in c["sets"]:
            ms = M.member_set(c["R"], which)
            kinds = [m[0] for m in ms]
            assert kinds == {"noise": ["noise"], "momentum": ["momentum"], "mixed": ["random", "noise", "momentum"],
                             "mixed_reversed": ["momentum", "noise", "random"]}[which], (name, which)
            assert len(ms) <= 4  # MAX_MEMBERS
            fixed = sum(m[1] for m in ms if m[0] == "random")
            assert fixed < c["pool"], (name, which)  # (bk_set_agents: the others' orders need pool slots)
            if which.startswith("mixed") and c["R"] > 1:  # the RandomAgents' orders reach the pool's last register
                assert fixed > 64 * (c["R"] - 1), (name, which)
            # disjoint trader ids: the GPU test tells the members' orders apart by them
            spans = [(0, m[1]) if m[0] == "random" else (m[1], m[1] + m[2]) for m in ms]
            for i, (a0, a1) in enumerate(spans):
                for b0, b1 in spans[i + 1:]:
                    assert a1 <= b0 or b1 <= a0, (name, which, spans)


def test_importing_the_table_initialises_no_gpu_runtime():
    code = ("import sys; sys.path.insert(0, 'tests'); import members_ingress_cases; "
            "print(sorted(m for m in sys.modules if m.split('.')[0] in ('torch', 'bourse_amd', 'ctypes')))")
    out = subprocess.run([sys.executable, "-c", code], cwd=M.ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "[]", out
