"""The kernel case table (tests/kernel_cases.py) names every shipped instantiation of profiles/kernel_isa_baseline.json, and
nothing else, with a well-formed configuration: a new instantiation without a GPU parity case fails here, on the CPU."""
import subprocess
import sys

import kernel_cases as K


def test_the_table_names_exactly_the_baseline_instantiations():
    missing, extra = K.compare_with_baseline(K.CASES, K.baseline_kernels())
    assert not missing, f"baseline instantiations without a case in tests/kernel_cases.py: {missing}"
    assert not extra, f"cases for instantiations the baseline does not list: {extra}"


def test_a_new_baseline_instantiation_without_a_case_fails_the_comparison():
    kernels = K.baseline_kernels() | {"k_step_batch<16, false, false>"}
    assert K.compare_with_baseline(K.CASES, kernels) == (["k_step_batch<16, false, false>"], [])
    names = set(K.CASES) - {"k_step_decode<4>"}
    assert K.compare_with_baseline(names, K.baseline_kernels()) == (["k_step_decode<4>"], [])
    assert K.compare_with_baseline(set(K.CASES) | {"k_gone<1>"}, K.baseline_kernels()) == ([], ["k_gone<1>"])


def test_every_entry_is_well_formed():
    for name, c in K.CASES.items():
        assert c["name"] == name
        assert c["unreachable"] is None, (name, "every instantiation is reachable from the public API")
        assert c["pool"] == 64 * c["R"] and c["R"] in K.POOLS, name
        assert c["flow"] in K.FLOWS, name
        assert len(c["launches"]) >= 2 and len(set(c["launches"])) >= 2 and min(c["launches"]) >= 1, name
        assert all(k.startswith("BOURSE_AMD_") and isinstance(v, str) for k, v in c["knobs"].items()), name
        args = [a.strip() for a in name.split("<")[1].rstrip(">").split(",")]
        if c["flow"] == "run":
            assert c["agents"] in K.AGENTS[1:], name
            assert c["pipeline"] is None or c["pipeline"] in K.REQUESTS, name
            assert c["kind"] in K.KINDS and c["parts"] >= 1, name
            assert c["launches"][0] % 2 == 1, (name, "the filler agents' orders rest after an odd number of steps")
            if c["parts"] > 1:  # uneven parts whose boundaries round down to multiples of 4
                sizes = K.part_sizes(c["units"], c["parts"])
                assert len(set(sizes)) > 1 and min(sizes) > 0, (name, sizes)
                if c["kind"] == "split":
                    assert c["split_parts"] == (c["parts"], 64), name
                else:
                    assert c["wave_options"][1] == c["parts"], name
            per = K.PER_BLOCK.get(K.family(name))
            if per:  # the last workgroup of the kernel's grid (of the last part) is partial
                books = c["units"] * (len(K.TICKS) if c["markets"] and per == 4 else 1)
                last = K.part_sizes(books, c["parts"])[-1] if K.family(name) not in K.PER_BLOCK or c["parts"] > 1 else books
                assert last % per != 0, (name, last, per)
        elif c["flow"] == "host":
            assert c["agents"] is None and c["mods_from"] is not None, name
            assert args[1] == ("true" if c["markets"] else "false") and args[2] == ("true" if c["chunks"] else "false"), name
        else:
            assert c["agents"] == "random" and not c["markets"], name
        # the template's arguments follow from the configuration
        fam = K.family(name)
        if fam in ("k_step_batch", "k_step_batch_log"):
            assert args[1] == ("true" if c["markets"] else "false"), name
            assert c["log"] == (fam == "k_step_batch_log"), name
            if fam == "k_step_batch":
                assert args[2] == ("true" if c["agents"].startswith("members") else "false"), name
        if fam in ("k_run_wave", "k_agents_fsm", "k_agents_wave", "k_agents_mixed", "k_agents_mixed_wave", "k_run_mixed"):
            assert c["agents"].endswith("_table") == (len(args) > 1 and args[-1] == "true"), name
        if fam == "k_agents_mixed_lanes":
            assert args[1] == ("true" if c["markets"] else "false"), name
            assert c["agents"].endswith("_table") == (len(args) > 2), name
        if fam == "k_step_decode":
            assert c["knobs"] == {"BOURSE_AMD_STEP_DECODE": "1"} and c["kind"] == "wave_split" and not c["log"], name


def test_importing_the_table_initialises_no_gpu_runtime():
    code = "import sys; sys.path.insert(0, 'tests'); import kernel_cases; print(sorted(m for m in sys.modules if m.split('.')[0] in ('torch', 'bourse_amd', 'ctypes')))"
    out = subprocess.run([sys.executable, "-c", code], cwd=K.ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "[]", out
