"""The ledger of tests/gp_sweep_matrix.py against the sources and the oracle (no GPU).

* the dispatch lists of ``sl_common.h``, ``sl_gp_small.hip`` and ``sl_gp.hip`` are the lists the ledger declares, the
  constants and the struct layouts its rules use are the sources';
* every instantiation those lists compile has exactly one entry; the existing tests the ledger names exist and
  assert the note the ledger records;
* every new case selects what it claims under the restated rules, on 256 compute units and on 128;
* the rules are pinned against the seven cases of ``tests/test_gpu_configs.py`` (16 / 4 wavefronts on an MI355X);
* every case is well posed on the oracle alone: its mask on the compared cells has both classes, 5 % at least."""

import inspect
import os
import re
import sys

import numpy as np
import pytest

import cases
import gp_sweep_matrix as gm
from conftest import ROOT

CSRC = os.path.join(ROOT, "safe_learning_amd", "csrc")
UNITS = {"sl_hip.h": os.path.join(ROOT, "include", "sl_hip.h")}


def _source(name):
    with open(UNITS.get(name, os.path.join(CSRC, name))) as handle:
        text = handle.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def dispatch_lists(text):
    """The template arguments of every ``sl_with_dim<...>(`` call, in source order."""
    return [tuple(v.strip() for v in m.group(1).split(","))
            for m in re.finditer(r"\bsl_with_dim\s*<([^<>]*)>\s*\(", text)]


def _one(pattern, text, flags=0):
    found = re.findall(pattern, text, flags)
    assert len(found) == 1, (pattern, found)
    return found[0]


def parsed_constants():
    """What the sources say about every name of gm.CONSTANTS."""
    small, gp, common, hip, model = (_source(n) for n in ("sl_gp_small.hip", "sl_gp.hip", "sl_common.h", "sl_hip.h",
                                                          "sl_model.h"))
    out = {}
    for name in ("WAVES_MIN", "WAVES_MAX", "WAVES_TOP", "WAVES_TINY"):
        out[name] = int(_one(r"constexpr int [^;]*\b%s = (\d+)" % name, small))
    w = _one(r"const int weight\[4\] = \{(\d+), (\d+), (\d+), fits\(WAVES_TOP, true\) \? (\d+) : "
             r"\(fits\(WAVES_MAX, true\) \? (\d+) : (\d+)\)\};", small)
    out["WEIGHTS"] = (int(w[0]), int(w[1]), int(w[2]), (int(w[3]), int(w[4]), int(w[5])))
    out["COUNTER_EXTRA"] = int(_one(r"ntiles \* \(weight\[k\] \+ \(k == 1 \? (\d+) : 0\)\) / per_round", small))
    rounds = re.findall(r"ntiles (?:<|>=) \(int64_t\)(\d+) \* ctx->num_cu \* WAVES_TOP", small)
    assert len(rounds) == 2 and len(set(rounds)) == 1, rounds          # the round-cost rule and the large-sweep rule
    out["ROUNDS"] = int(rounds[0])
    cap = _one(r"return (\d+) \* (\d+) - \(general \? sizeof\(SlTriLds<true>\) : 0\) - (\d+);", small)
    out["LDS_BYTES"], out["LDS_RESERVE"] = int(cap[0]) * int(cap[1]), int(cap[2])
    assert "%d * %d" % (int(cap[0]), int(cap[1])) in _one(r"if \(fixed \+ sizeof\(double\) \* xs_max <= ([^)]+)\) return", gp)
    out["SMALL_PAD_MAX"] = int(_one(r"h\.n_pad > (\d+) \|\| h\.n_pad % 16", small))
    pad, above = _one(r"gp_heads\[h\]\.n_pad != (\d+) \|\| ctx->gp_heads\[h\]\.n <= (\d+)\) return SL_DECLINED", gp)
    out["ONE_PANEL_PAD"], out["ONE_PANEL_ABOVE"] = int(pad), int(above)
    out["SMALL_HEAD_MAX"] = int(_one(r"if \(n <= (\d+)\) return 0;\s*return 2;", gp))
    out["SL_GP_SLABS_PER_CHUNK"] = int(_one(r"#define SL_GP_SLABS_PER_CHUNK (\d+)", gp))
    for name in ("SL_MAX_STATE_DIM", "SL_MAX_INPUT_DIM", "SL_MAX_SIMPLICES", "SL_KERNEL_MAX_FACTORS"):
        out[name] = int(_one(r"#define %s\s+(\d+)" % name, hip))
    for name in ("SL_TRI_CODES", "SL_TRI_MAXCAND"):
        out[name] = int(_one(r"#define %s\s+(\d+)" % name, model))
    assert re.search(r"template <bool ON> struct SlTriLds \{ SlTri t\[2\]; \};", common)
    return out


def struct_members(text, name):
    """[(type, member, dimensions)] of ``struct name { ... }`` / ``typedef struct name { ... }``."""
    body = _one(r"struct %s \{(.*?)\n\}" % name, text, re.S)
    out = []
    for statement in body.split(";"):
        statement = " ".join(statement.split())
        if not statement:
            continue
        ctype, rest = re.match(r"((?:const )?\w+\*?) (.*)", statement).groups()
        for item in rest.split(","):
            m = re.match(r"\s*(\w+)((?:\[[^\]]+\])*)\s*$", item)
            out.append((ctype, m.group(1), tuple(re.findall(r"\[([^\]]+)\]", m.group(2)))))
    return out


def test_ledger_lists_are_the_dispatchers_lists():
    for unit in sorted(gm.DISPATCH):
        declared = [values for _, values in gm.DISPATCH[unit]]
        assert dispatch_lists(_source(unit)) == declared, \
            "%s: the sl_with_dim lists changed - update tests/gp_sweep_matrix.py (DISPATCH and the entries)" % unit
    gp = _source("sl_gp.hip")
    for name, values in gm.CFG.items():
        assert tuple(int(v) for v in _one(r"constexpr int %s\[2\] = \{(\d+), (\d+)\};" % name, gp)) == values
    # the lists feed the template parameters in the order the ledger reads them
    small = _source("sl_gp_small.hip")
    assert "k_gp_small<GENERAL, DT, MT, (f & 2) != 0, W, (f & 1) != 0>" in small
    assert "const int flags = (alds ? 2 : 0) | (sl_has_other_kernels(ctx) ? 1 : 0);" in small
    assert "launch_cfg<8, 4, 4, d == 0, d, d != 0 ? 1 : 0, true>(ctx, g)" in gp
    assert "if constexpr (DT > 0) rc = sl_with_dim<WAVES_MAX, WAVES_TOP, WAVES_TINY, WAVES_MIN>(waves, launch);" in small
    assert "std::integral_constant<int, d != 0 ? 1 : 0>()" in _source("sl_common.h")
    assert sum(len(v) for v in gm.instantiations().values()) == 105


def test_list_parser_sees_an_edited_list():
    """An instantiation added to, or dropped from, a dispatcher changes what the parser returns."""
    text = _source("sl_gp_small.hip")
    assert dispatch_lists(text.replace("sl_with_dim<3, 2, 1, 0>", "sl_with_dim<3, 2, 0>", 1))[0] == ("3", "2", "0")
    assert dispatch_lists(text.replace("sl_with_dim<WAVES_MIN>", "sl_with_dim<WAVES_MIN, WAVES_TINY>")) != dispatch_lists(text)
    common = _source("sl_common.h")
    assert dispatch_lists(common.replace("sl_with_dim<2, 0>", "sl_with_dim<2, 3, 0>")) != dispatch_lists(common)


def test_constants_are_the_sources():
    parsed = parsed_constants()
    assert parsed == gm.CONSTANTS
    small = _source("sl_gp_small.hip")
    assert _one(r"constexpr int tri_offset\(int I\) \{ return ([^;]+); \}", small) == "I * (I + 1)"
    assert all(gm.tri_offset(i) == i * (i + 1) for i in range(17))
    assert _one(r"constexpr int KERNEL_DOUBLES = ([^;]+);", small) == "(int)((sizeof(sl_gp_kernel) + 15) / 16) * 2"
    # the layouts behind sizeof(SlTriLds<true>) and sizeof(sl_gp_kernel)
    assert struct_members(_source("sl_model.h"), "SlTri") == gm.TRI_MEMBERS
    hip = _source("sl_hip.h")
    assert struct_members(hip, "sl_grid_desc") == gm.GRID_DESC_MEMBERS
    assert struct_members(hip, "sl_gp_kernel_factor") == gm.KERNEL_FACTOR_MEMBERS
    assert struct_members(hip, "sl_gp_kernel") == gm.KERNEL_MEMBERS
    assert gm.tri_lds_bytes() == 2 * 19056 and gm.kernel_doubles() == 138
    # ... and a moved constant moves them
    assert gm.tri_lds_bytes(dict(gm.CONSTANTS, SL_MAX_SIMPLICES=33)) > gm.tri_lds_bytes()
    assert gm.kernel_doubles(dict(gm.CONSTANTS, SL_KERNEL_MAX_FACTORS=9)) > gm.kernel_doubles()


def test_the_launchers_rules_are_the_ledgers():
    """The statements the restated rules follow, where the sources state them."""
    small, gp, common = _source("sl_gp_small.hip"), _source("sl_gp.hip"), _source("sl_common.h")
    for text in (
            "small += (size_t)((p * h.n_pad + 1) & ~1) + (size_t)((h.n_pad * h.dout + 1) & ~1) +",
            "tri += (size_t)tri_offset((h.n + 15) / 16) * 128;",
            "auto scratch_of = [&](int waves) { return (size_t)waves * 64 * (1 + 2 * d); };",
            "return sizeof(double) * (small + (with_tri ? tri : 0) + scratch_of(waves)) <= cap;",
            "return w == WAVES_MIN || wcap < 0 || (w > WAVES_MIN && w <= wcap) || (w == WAVES_TINY && wcap == WAVES_TINY);",
            "const int sizes[4] = {WAVES_TINY, WAVES_MIN, WAVES_MAX, WAVES_TOP};",
            "if (!allowed(sizes[k]) || !fits(sizes[k], false)) continue;",
            ": ((ntiles + per_round - 1) / per_round) * weight[k];",
            "if (best < 0 || cost < best) { best = cost; waves = sizes[k]; }",
            "} else if (DT > 0 && allowed(WAVES_MAX) && fits(WAVES_MAX, alds)) {",
            "if (alds && fits(WAVES_TOP, true)) {",
            "} else if (!(alds && waves == WAVES_MAX) && fits(WAVES_TOP, false)) {",
            "return small + (size_t)gps::WAVES_MIN * 64 * (1 + 2 * d);",
            "if (ctx->env.gp_small == 0) return false;"):
        assert text in small, text
    for text in (
            "static inline int cfg_panel_rows(int cfg) { return 16 * kCfgR[cfg != 0] * kCfgW[cfg != 0]; }",
            "const int n_pad = ((n + rp - 1) / rp) * rp;",
            "if (ctx->env.gp_cfg >= 0) return ctx->env.gp_cfg;",
            "if (!sl_has_other_kernels(ctx) || !sl_gp_small_supports(ctx, g.model)) return SL_DECLINED;",
            "if (ctx->gp_cfg != 0 || sl_has_other_kernels(ctx) || !sl_gp4_supports(g.model) || ctx->env.gp4_one_panel == 0)",
            "if (ctx->gp_cfg != 0 || !sl_gp_small_supports(ctx, g.model)) return SL_DECLINED;",
            "if (ctx->gp_cfg != 2 || sl_has_other_kernels(ctx) || !sl_gp4_supports(g.model)) return SL_DECLINED;",
            "if (ctx->gp_cfg == 0) return SL_DECLINED;",
            "const size_t fixed = sizeof(double) * (2 * SL_GP_SLABS_PER_CHUNK * 4 * 64 + 8 * 64 +",
            "8 * 16 * SL_GP_DOUT_MAX + 2 * 64 * SL_D + 2 * 8);",
            "#define SL_GP_DOUT_MAX SL_MAX_STATE_DIM",
            "const int variant = sl_model_is_general(g.model) ? 0 : sl_dim_variant_of(g.model);",
            "return ctx->gp_cfg == 0 ? gp_sweep_shape<0>(ctx, g) : gp_sweep_shape<1>(ctx, g);"):
        assert text in gp, text
    chain = _one(r"for \(auto launch : \{([^}]+)\}\)", gp)
    assert tuple(v.strip() for v in chain.split(",")) == gm.CHAIN
    assert "if (M.m.policy.m == 1 && M.m.grid.d >= 1 && M.m.grid.d <= 4) return M.m.grid.d;" in common
    assert ("return M.m.value.kind != SL_V_QUADRATIC || M.m.policy.kind == SL_POLICY_TRI ||" in common and
            "M.m.lipschitz.lv_kind == SL_LIP_ABS_GRAD || M.m.lipschitz.lv_kind == SL_LIP_NORM_GRAD;" in common)
    assert "return !sl_model_is_general(model) && sl_dim_variant_of(model) >= 1;" in _source("sl_gp4.hip")
    kernels = _source("sl_kernels.hip")
    assert "if (e->gp_cfg == 1 || e->gp_cfg > 3) e->gp_cfg = -1;" in kernels
    for name in gm.SWITCHES:
        assert 'env_int("%s")' % name in kernels, name
    assert [gm.sl_dim_variant_of(d, 1) for d in range(7)] == [0, 1, 2, 3, 4, 0, 0] and gm.sl_dim_variant_of(2, 2) == 0
    assert gm.flavour_of(True, 3, 1) == (1, 0, 0) and gm.flavour_of(False, 3, 1) == (0, 3, 1)
    assert gm.flavour_of(False, 2, 2) == (0, 0, 0) and gm.flavour_of(True, 2, 1) == (1, 2, 1)
    # the notes are the launchers'
    assert '"k_gp_small<general=%d, d=%d, m=%d, Linv in %s, %d wavefronts> (%d head(s))"' in small
    assert '"k_gp_sweep<W=%d, R=%d, CB=%d, general=%d, d=%d, m=%d, xs_global=%d>"' in gp


def test_every_instantiation_has_exactly_one_entry():
    compiled = gm.instantiations()
    listed = {}
    for e in gm.ENTRIES:
        listed.setdefault(e["kernel"], []).append(e["params"])
    assert set(listed) == set(compiled)
    for kernel, params in compiled.items():
        assert sorted(listed[kernel]) == sorted(params), (kernel, set(listed[kernel]) ^ params)
    assert {e["kind"] for e in gm.ENTRIES} <= {"existing", "new", "unreachable"}
    assert len(gm.ENTRIES) == 105


def _bench_case(flags):
    sys.path.insert(0, ROOT)
    import bench
    argv = ["--config", flags["config"]]
    for key, val in flags.items():
        if key != "config":
            argv += ["--" + key.replace("_", "-"), str(val)]
    return bench.build_workload(bench.parse_args(argv))[2]


def test_rules_are_pinned_against_the_seven_benchmark_cases():
    """tests/test_gpu_configs.py's seven cases run 16 / 4 wavefronts on an MI355X, and 12 / 8 under their cap: the
    restated rules give exactly that, with the flavour, placement and head count the ledger records."""
    seen = set()
    for test, flags, env, params, heads in gm.CONFIG_CASES:
        case = _bench_case(flags)
        tiles = (int(np.prod(case["num_points"])) + 63) // 64
        assert gm.select(gm.describe(case), env, tiles, gm.MI355X_CUS) == gm.small_note(params, heads), (test, env)
        unrestricted, capped = (16, 12) if "sixteen" in test else (4, 8)
        assert params[4] == (capped if env else unrestricted) and env in ({}, {"SL_GP_SMALL_WAVES": str(capped)})
        seen.add((test, bool(env)))
    assert len(seen) == 14


def test_existing_tests_exist_and_assert_the_note():
    import test_gpu_configs
    for e in gm.entries("existing"):
        module, _, name = e["existing"].partition("::")
        assert module == "tests.test_gpu_configs"
        function, _, param = name.partition("[")
        test = getattr(test_gpu_configs, function)
        marks = [m for m in test.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and marks[0].args[0] == "flags"
        index = int(re.fullmatch(r"flags(\d+)\]", param).group(1))
        assert marks[0].args[1][index] == e["flags"], e["existing"]
        # the test holds every launch's note to the ledger's, in full
        assert "gp_sweep_matrix.config_note(flags, cap)" in inspect.getsource(test)
        assert gm.config_note(e["flags"], e["env"].get("SL_GP_SMALL_WAVES")) == e["expect"]


@pytest.mark.parametrize("num_cu", [256, 128])
def test_new_cases_select_what_they_claim(num_cu):
    """On an MI355X's 256 compute units and on half as many (a smaller part must not move a case to another
    kernel without this test noticing; a LARGER part needs larger round-cost grids - sweep_range says so)."""
    for e in gm.entries("new"):
        c = e["case"]
        assert e["expect"] == (gm.small_note(e["params"], len(gm.model_of(c)["heads"])) if e["kernel"] == "k_gp_small"
                               else gm.sweep_note(e["params"]))
        assert gm.select(gm.model_of(c), c["env"], gm.ntiles(c, num_cu), num_cu) == e["expect"], gm.entry_id(e)
        assert c["n_gp"] % 16 and int(np.prod(c["num_points"])) % 64, "padded rows and a ragged last tile"
        lo, hi = gm.sweep_range(c, num_cu)
        assert lo % 64 == 0 and 0 <= lo < hi == int(np.prod(c["num_points"]))
        if c["waves"] not in (None, 8):
            assert "SL_GP_SMALL_WAVES" not in c["env"]            # the launcher's own rule, no switch
            assert lo > 0 or num_cu == 256
        if e["anchor"] is not True:
            a = e["anchor"]
            assert e["kernel"] == "k_gp_small" and a["env"] == gm.EIGHT
            assert (a["family"], a["num_points"], a["n_gp"], a["kernels"]) == (c["family"], c["num_points"], c["n_gp"], c["kernels"])
            assert gm.sweep_range(a, num_cu) == (lo, hi)
            note = gm.select(gm.model_of(a), a["env"], gm.ntiles(a, num_cu), num_cu)
            assert ", 8 wavefronts>" in note and note.split(", Linv")[0] == e["expect"].split(", Linv")[0]
        if e["down"] is not None:
            env, family = e["down"]
            assert gm.select(gm.model_of(c), env, gm.ntiles(c, num_cu), num_cu).startswith(family.rstrip("<")), gm.entry_id(e)
    # the pairs whose placement differs between the two wave counts are kept
    pairs = [e for e in gm.entries("new", "k_gp_small") if e["anchor"] is not True and not e["params"][3] and
             "Linv in LDS" in gm.select(gm.model_of(e["anchor"]), gm.EIGHT, gm.ntiles(e["anchor"], num_cu), num_cu)]
    assert len(pairs) >= 8, [gm.entry_id(e) for e in pairs]


def _distinct_models():
    seen, out = set(), []
    for e in gm.entries("new"):
        c = e["case"]
        key = (c["family"], tuple(c["num_points"]), c["n_gp"], c["kernels"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_the_cheap_description_of_a_case_is_its_description():
    for c in _distinct_models():
        if int(np.prod(c["num_points"])) <= 4096 or c["n_gp"] == 90:
            assert gm.describe(gm.make(c)) == gm.model_of(c), gm.case_id(c)


def test_no_instantiation_is_unreachable_and_the_candidates_are_reached():
    """The rules rule nothing out: the table d = 0 flavours take sum-of-products heads (a stack of one head on a 1-D
    table model), and ``gp_sweep_xs_global`` takes a pendulum model once SL_GP_CFG=3 keeps k_gp_sweep4 away.  Each
    statement fails when the constant it rests on moves."""
    for e in gm.entries("unreachable"):
        assert e["check"](gm.CONSTANTS), e["reason"]
    assert not gm.entries("unreachable")
    table0 = gm.model_of(gm.case("table1d", [1500], 90, True))
    assert gm.select(table0, {}, 24, 256) == gm.small_note((1, 0, 0, 1, 8, 1), 1)
    assert gm.select(table0, {}, 24, 256, dict(gm.CONSTANTS, LDS_BYTES=48 * 1024)).startswith("k_gp_sweep<")
    xs2 = gm.model_of(gm.XS_CASES[2])
    assert gm.select(xs2, gm.CFG3, 27, 256) == gm.sweep_note((8, 4, 4, 0, 2, 1, 1))
    assert gm.select(xs2, {}, 27, 256) == "k_gp_sweep4"                       # gp4_cfg2 is asked first
    assert gm.select(xs2, gm.CFG3, 27, 256, dict(gm.CONSTANTS, LDS_BYTES=192 * 1024)) == gm.sweep_note((8, 4, 4, 0, 2, 1, 0))
    assert gm.select(gm.model_of(gm.XS_CASES[2] | dict(n_gp=3000)), gm.CFG3, 27, 256) == gm.sweep_note((8, 4, 4, 0, 2, 1, 0))


_MASKS = {}


def oracle_records(c):
    """(case dict, compared cells, the oracle's records there, cells whose threshold and decrease have one value):
    computed once per model, shared with the GPU tests and left unchanged."""
    key = (c["family"], tuple(c["num_points"]), c["n_gp"], c["kernels"])
    if key not in _MASKS:
        made = gm.make(c)
        olyap = cases.oracle_lyapunov(made)
        cells = gm.compared_cells(c)
        ref = cases.oracle_cell_records(olyap, cells)
        ok = np.ones(len(cells), dtype=bool)
        if made.get("V", {}).get("kind") == "table":
            # |grad V| and V are simplex dependent on the lines of the table grid: the cell itself, then its successor
            from test_gpu_lyapunov import _on_table_face
            otri = olyap.lyapunov_function
            ok = ~_on_table_face(otri, olyap.discretization.index_to_state(cells))
            ok &= ~_on_table_face(otri, ref[:, 2:2 + made["d"]])
        for array in (cells, ref, ok):
            array.setflags(write=False)
        _MASKS[key] = (made, cells, ref, ok)
    return _MASKS[key]


@pytest.mark.parametrize("c", _distinct_models(), ids=lambda c: gm.case_id(dict(c, env={}, waves=None)))
def test_cases_are_well_posed_on_the_oracle(c):
    made, cells, ref, ok = oracle_records(c)
    assert np.isfinite(ref).all()
    neg = ref[ok, 0] < ref[ok, 1]
    print("%s: %d compared cells, %d on table lines, %.1f %% pass the decrease check" % (
        gm.case_id(c), len(cells), int((~ok).sum()), 100.0 * neg.mean()))
    assert 0.05 <= neg.mean() <= 0.95
    # left out: the cells on the boundary lines of a table grid (the first block and the last among them); beside
    # them next to nothing
    states = np.asarray(cases.oracle.GridWorld(made["limits"], made["num_points"]).index_to_state(cells))
    edge = (np.abs(np.abs(states) - 1.0) < 1e-12).any(axis=1)
    assert (~ok & ~edge).sum() <= 0.02 * len(cells)
    assert (ref[:, 2 + made["d"]:] > 0).all()                          # a posterior with an error bound
