"""Regenerate profiles/README.md: one row per shipped kernel (source file, the configuration that
measures it, ms, fraction of its roof, the counter / A-B files behind the number) and a list of what
else is in profiles/.  Reads profiles/r06_configs.jsonl (tools/bench_configs.sh), the headline line
profiles/r06_bench_driver_command.log, profiles/early_bench_headline.jsonl, profiles/blocks_ab_headline.jsonl and
profiles/meanpass_ab_headline.jsonl, profiles/variance_floor_ab.jsonl, profiles/pmc_traffic.json and
profiles/pmc_valu.json.

    python tools/profiles_index.py"""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = os.path.join(ROOT, "profiles")

# kernel -> (source, configuration that measures it, files with the evidence)
KERNELS = [
    ("k_gp_predecide + k_gp_mean_open + k_gp_sweep4", "csrc/sl_gp4_predecide.hip, csrc/sl_gp4_mean.hip, csrc/sl_gp4.hip", "C4", "open_list.md (the mean pass from a compacted list of the open "
     "blocks: resources, listings, A/B open_list_ab.jsonl, trace open_list_kernel_stats.md); predecide.md (blocks decided before the mean from a "
     "first-order Taylor expansion with an RKHS bound of its remainder: CPU counts, listings, A/B predecide_ab.jsonl); variance_floor.md (the variance floor in the lower bound: listings, CPU prediction floor_cpu_counts.txt, device stage counts, "
     "A/B variance_floor_ab.jsonl, kernel trace, upload cost); shared_block_source.md (one source for both kernels' block arithmetic); meanpass_ab_headline.jsonl (parent / mean kernel, alternating on one box), meanpass_before.md (the source pass of the parent split), "
     "meanpass_kernel_stats.md (both kernels, matrix pipe, stage counts, flush cost), meanpass_other_lines.txt; packed 16-cell blocks before it: blocks_ab_headline.jsonl (parent / 16-cell blocks, alternating on one box), blocks_other_lines.txt, blocks_kernel_stats.md, "
     "blocks_stage_counts.txt, blocks_pmc_128.txt, blocks_little_skipped.txt, blocks_cpu_counts.txt (tools/early_block_counts.py); the 64-cell early decision before it: early_ab_headline.jsonl (parent / early / plain, interleaved on one box), early_kernel_stats.md, early_pmc_48.txt, early_pmc_128.txt, "
     "early_stage_counts.txt, early_ab_other_lines.jsonl, early_dump_outputs.txt, early_little_skipped.txt; the plain instantiation (every panel of every tile): r06_kernel_stats.md, r06_pmc_48.txt, r06_pmc_128.txt, r05_pmc_l2_64.txt, pmc_traffic.json; "
     "A/B: dropped/r06_gp4_alias_ab.txt (phases; every factor read an L2 hit: -1 %), dropped/r06_gp4_seeds_nontemporal_ab.txt, dropped/r06_gp4_seed_latency_ab.txt, r05_gp4_diag_ab.txt"),
    ("k_gp_sweep4 (n = 512, 1024 tiles)", "csrc/sl_gp4.hip", "C2", "r06_C2_kernel_stats.md, r05_C2_ab.txt; dropped/r06_gp4_stagger_ab.txt (tile-count series at 512 points)"),
    ("k_gp_sweep4 + k_nn_check_mfma", "csrc/sl_gp4.hip, csrc/sl_nn.hip", "C3", "r06_C3_kernel_stats.md, r04_C3_kernel_stats.md; r06_box_variance_ab.txt (270.5 ms on another box, "
     "round-5 library 270.9 ms beside it)"),
    ("k_gp_small (one head, table V and policy)", "csrc/sl_gp_small.hip", "C2-table-large", "r06_C2-table-large_kernel_stats.md, pmc_valu.json; r06_gp_small_lds_ab.txt (factor in LDS beside sixteen wavefronts, pass order)"),
    ("k_gp_small (small grid)", "csrc/sl_gp_small.hip", "C2-table", "pmc_valu.json; r06_gp_small_lds_ab.txt (four-wavefront workgroups)"),
    ("k_gp_small (two-head stack)", "csrc/sl_gp_small.hip", "C2-table-stack", "pmc_valu.json; r04_gp_small_tickets_ab.txt"),
    ("k_gp_small (notebook kernels)", "csrc/sl_gp_small.hip", "C2-notebook", "r06_C2-notebook_kernel_stats.md, pmc_valu.json"),
    ("k_det_rows + k_finalize_dev", "csrc/sl_det_rows.hip, csrc/sl_level.hip", "C4-lin", "pmc_valu.json, r04_C4-lin_kernel_stats.md, r04_C4-lin_pmc.txt"),
    ("k_det_sweep (Euler cart-pole)", "csrc/sl_kernels.hip", "C4-det", "pmc_valu.json"),
    ("k_det_sweep (table V)", "csrc/sl_kernels.hip", "C2-table-det", "r06_C2-table-det_kernel_stats.md, pmc_valu.json; r06_gen_waves_ab.txt (wavefronts per SIMD by launch bound)"),
    ("k_det_sweep (1-D toy)", "csrc/sl_kernels.hip", "C1", ""),
    ("k_bellman_cached (max; sweeps 2 .. n of a loop)", "csrc/sl_succ.hip", "C5", "r06_C5_kernel_stats.md, r06_C5_cached_traffic.txt, r06_C5_pmc.txt; the line's "
     "`uncached_sweep` / `first_sweep_ms` = k_bellman4s + k_bellman_lookup (csrc/sl_bellman4.hip), pmc_valu.json[C5-lookup]"),
    ("k_bellman_cached (policy) + k_succ_policy_miss", "csrc/sl_succ.hip", "C5-policy", "r06_C5-policy_kernel_stats.md; r06_gen_waves_ab.txt (k_succ_select)"),
]


def load_lines(name):
    out = {}
    try:
        with open(os.path.join(P, name)) as f:
            for line in f:
                line = line.strip()
                if line.startswith("{"):
                    d = json.loads(line)
                    if "result" in d:                      # an A/B file: {"line", "side", "run", "result"}
                        if d["line"] != "headline" or d["side"] != "change":
                            continue
                        d = d["result"]
                    out[d["config"].get("name", "C4")] = d
    except OSError:
        pass
    return out


def main():
    lines = load_lines("r06_configs.jsonl")
    lines.update(load_lines("r06_bench_driver_command.log"))
    lines.update(load_lines("early_bench_headline.jsonl"))      # the headline with the early tile decision
    lines.update(load_lines("blocks_ab_headline.jsonl"))        # ... on packed 16-cell blocks (the last line: this commit)
    lines.update(load_lines("meanpass_ab_headline.jsonl"))      # ... with the mean kernel in front (the last line: this commit)
    lines.update(load_lines("variance_floor_ab.jsonl"))         # ... with the variance floor in the lower bound
    try:
        valu = json.load(open(os.path.join(P, "pmc_valu.json")))
    except (OSError, ValueError):
        valu = {}
    rows = ["| kernel(s) | source (safe_learning_amd/) | configuration (`bench.py --config`) | ms per step | kernel ms | roof | fraction | evidence (profiles/) |",
            "|---|---|---|---|---|---|---|---|"]
    for kernel, source, cfg, files in KERNELS:
        d = lines.get(cfg)
        if d is None:
            rows.append("| `%s` | %s | %s | - | - | - | - | %s |" % (kernel, source, cfg, files))
            continue
        r = d["roofline"]
        frac = "%.3f" % r["frac"] if r.get("frac") is not None else "-"
        bound = r["bound"]
        if bound == "valu":
            extra = [k for k in ("hbm_frac", "mfma_frac") if k in r]
            if extra:
                frac += " (%s %.3f)" % (extra[0].replace("_frac", ""), r[extra[0]])
        rows.append("| `%s` | %s | %s | %.4g | %.4g | %s | %s | %s |" % (
            kernel, source, cfg, d["ms_per_step"], r["kernel_ms"], bound, frac, files))
    listing = sorted(os.listdir(P))
    by_round = {}
    for name in listing:
        key = name.split("_")[0] if name[:1] == "r" and name[1:3].isdigit() else "other"
        by_round.setdefault(key, []).append(name)
    text = ["# profiles/ — index", "",
            "Generated by `tools/profiles_index.py` from `r06_configs.jsonl` (one `bench.py` line per configuration,",
            "`tools/bench_configs.sh`), `r06_bench_driver_command.log` / `early_bench_headline.jsonl` (the headline command), `pmc_traffic.json` and",
            "`pmc_valu.json` (counter passes of `tools/profile_r06.sh`, tied to the kernel sources by sha256).",
            "One MI355X.  `roof`: `mfma` = 78.6 TFLOP/s FP64 matrix pipe (algorithmic flops, SURVEY 8d), `hbm` = 8 TB/s,",
            "`valu` = share of the SIMDs' cycles that issue a vector-ALU instruction (in brackets: the byte or",
            "matrix-pipe fraction bench.py printed before round 5).  The headline's `mfma` fraction counts the algorithmic",
            "flops of ALL cells while `k_gp_sweep4` skips the variance panels its bounds decide: an effective rate",
            "(matrix pipe busy 0.687 of the SIMD-cycles, `early_pmc_128.txt`; DESIGN.md 5).", ""] + rows + [""]
    if valu:
        text += ["## Vector-ALU issue utilisation (`pmc_valu.json`)", "",
                 "| entry | kernel | issue utilisation | FP64 share of the vector instructions | matrix pipe busy | wave-cycles waiting |",
                 "|---|---|---|---|---|---|"]
        for key in sorted(valu):
            e = valu[key]
            text.append("| %s | `%s` | %.3f | %s | %s | %s |" % (
                key, e["kernel"][:60], e["valu_issue_utilisation"],
                "%.3f" % e["fp64_share_of_valu_instructions"] if "fp64_share_of_valu_instructions" in e else "-",
                "%.3f" % e["mfma_busy"] if "mfma_busy" in e else "-",
                "%.3f" % e["waves_waiting"] if "waves_waiting" in e else "-"))
        text.append("")
    text += ["## What else is here", "",
             "* `rNN_summary.md` (rounds 1-4): that round's narrative with every A/B it ran; `CHANGELOG.md` at the repo root is the digest.",
             "* `dropped/`: A/B runs (and one patch) of designs that were measured and NOT shipped.",
             "* `rNN_pytest_gpu*.log`, `rNN_smoke.log`: GPU test logs; `rNN_parity_exclusions.json`: what the table-lookup parity tests "
             "left out / membership-checked (`tests/exclusions.py`).",
             "* `r05_rocprofv3_memory_counters.txt`: every memory-side counter this rocprofv3 offers (there is none behind the fabric).",
             "* `early_*`: the early tile decision of `k_gp_sweep4` against its parent commit, everything from one visit of one box "
             "(DESIGN.md 4.1 \"Early tile decision\").",
             "* `meanpass_*`: the mean and the first decision of `k_gp_sweep4`'s block mode in `k_gp_mean_blocks` against the parent "
             "commit, one visit of one box (DESIGN.md 4.1).",
             "* `variance_floor.md`, `variance_floor_ab.jsonl`, `floor_cpu_counts.txt`: the variance floor in the lower bound of "
             "`k_gp_sweep4`'s early decision against the parent commit, one visit of one box (DESIGN.md 4.1).",
             "* `predecide.md`, `predecide_ab.jsonl`, `predecide_kernel_stats.md`: `k_gp_mean_lattice` / `k_gp_predecide` in front of `k_gp_mean_blocks` against the "
             "parent commit, alternating on one box, `predecide_kernel_stats.md`: the kernel traces of both sides (DESIGN.md 4.1 \"Deciding before the mean\").",
             "* `open_list.md`, `open_list_ab.jsonl`, `open_list_kernel_stats.md`: the open-block list behind `k_gp_predecide` and `k_gp_mean_open` against the "
             "parent commit, alternating on one box; the kernel traces of both sides (DESIGN.md 4.1 \"The open-block list\").",
             "* `r06_shard_balance.md`: the N = 2 / 4 / 8 shards of C4 and C5 timed one by one on one GPU (`tools/shard_balance.py`).",
             "* `r06_parity_report.md`: what the parity claims rest on, what is a definition, what is unpinned.",
             "* `r06_box_variance_ab.txt`: the round-5 library and the tree alternating on ONE box (C3, C4-lin, C4-det): boxes of the pool "
             "differ by 1-4 %, the libraries by < 0.3 %.",
             "* `rollout_roa.md`, `rollout_kernel_stats.md`: closed-loop rollouts (`k_rollout`, csrc/sl_rollout.hip) against the stepwise "
             "composition of the point evaluations and against the sweep of the same cells (`tools/rollout_probe.py`; DESIGN.md 4.2b).",
             "* `reward_rollout.md`: discounted returns (`k_reward_rollout`, `k_reward_fold`, csrc/sl_rollout.hip) against the stepwise "
             "composition of the point evaluations and against `k_rollout` over the same steps, with the registers / LDS of the new "
             "kernels (`tools/reward_rollout_probe.py`; DESIGN.md 4.2b).",
             "* `lyapunov_training.md`: training a LyapunovNetwork (`k_nn_loss`, `k_nn_param_grad`, csrc/sl_nn.hip): registers / LDS, "
             "the tolerance of the gradient comparisons and what it was measured from, one gradient against torch autograd "
             "(`tools/lyapunov_training_probe.py`).",
             "* `policy_training.md`: policy gradients of `future_values` (`k_action_gradient`, `k_policy_param_grad`, `k_tri_pg_*`, "
             "csrc/sl_policy_grad.hip): registers / LDS, the measured ratios of the GPU tests against their tolerances, a "
             "policy-improvement step at the notebook's shape and `sl_action_gradient` on a 64^4 grid beside an uncached "
             "policy-evaluation sweep (`tools/policy_training_probe.py`).",
             "* `safe_policy_training.md`: the Lyapunov penalty of `future_values`, differentiated (`k_sg_generate`, `k_sg_gemm`, "
             "`k_sg_epilogue`, csrc/sl_safe_grad.hip): registers / LDS / scratch, the measured ratios of the GPU tests against "
             "their tolerances, a safe policy-improvement step at the notebook's shape beside the unpenalised one and "
             "`sl_decrease_gradient` under a 1024-point RBF head against the FP64 matrix peak (`tools/safe_policy_probe.py`; "
             "DESIGN.md 4.5c).",
             "* `actor_critic.md`, `actor_critic_probe.jsonl`: actor-critic with a NeuralNetwork value function (`k_critic_batch`, "
             "csrc/sl_critic.hip, `sl_dense_param_grad`): registers / scratch / LDS, the measured ratios of the GPU tests against "
             "their tolerances, a critic and an actor step at the cart-pole notebook's batch and at 2^20 samples, split per call, "
             "beside torch autograd (`tools/actor_critic_probe.py`; DESIGN.md 4.5d).",
             "* `polynomial_dynamics.md`, `polynomial_probe.jsonl`: polynomial dynamics (`SL_DYN_POLYNOMIAL`, csrc/sl_polynomial.h): registers "
             "and scratch of the new instantiations, Van der Pol against the pendulum in the same kernels, and the eight entries of "
             "`pmc_valu.json` before and after the edit of the shared headers (`tools/polynomial_probe.py`; DESIGN.md 4.2c).",
             "* `polynomial_value.md`, `polynomial_value_probe.jsonl`: polynomial Lyapunov functions (`SL_V_POLYNOMIAL`, csrc/sl_poly_value.h, "
             "csrc/sl_poly_value.hip): registers, scratch and LDS of the seven new instantiations and of `k_eval_simple` before and after, the "
             "notebook's SOS candidate beside the LQR quadratic and a 101^2 table on the 2001 x 1501 pendulum grid, a quartic at 64^4 under "
             "the cart-pole, and `bench.py` against the parent's library on one box (`tools/polynomial_value_probe.py`, "
             "`tools/kernel_resources.py`; DESIGN.md 4.2d).",
             "* `gp_sample.md`: GP sample paths (`sl_gp_posterior_cov`, `sl_cholesky`, `sl_tri_solve`, `sl_tri_mult`, "
             "`sl_gp_sample_eval`, csrc/sl_gp_sample.hip): a first measurement of the four stages of `sample_gp_function` at "
             "N = 1 024 / 4 096 / 16 384 and of one sample function on 10^6 points beside `scipy.linalg.cholesky`, registers / LDS / "
             "scratch of the twelve new kernels, and the figures of the GPU tests against their allowances "
             "(`tools/gp_sample_probe.py`, `tools/kernel_resources.py`; DESIGN.md 4.2e).",
             "* `gp_likelihood.md`: GP hyper-parameters (`sl_gp_likelihood`, csrc/sl_gp_likelihood.hip): registers, private memory "
             "and LDS of the four new kernels, first timings of one likelihood call with and without the gradient at n = 130 / 1 024 / "
             "4 096, the gap between the two restatement searches that sets the allowance of the `optimize()` test, and figures of "
             "the GPU tests against their allowances (`tools/gp_likelihood_probe.py`, `tools/kernel_resources.py`; DESIGN.md 4.2f).",
             "* `gp_rollout.md`: closed-loop rollouts of a GP's posterior mean (`k_gp_rollout`, `k_gp_reward_rollout`, `k_gp_mean_points`, "
             "csrc/sl_gp_rollout.hip): registers, LDS and scratch of the new kernels, the fused `compute_roa` against the callable "
             "form, the measured (trajectory x step x training point) rate beside the derived one of the chunk rule, and the figures "
             "of the tests against their bounds (`tools/gp_rollout_probe.py`, `tools/kernel_resources.py`; DESIGN.md 4.2g).",
             "* `gp_posterior_truth.md`: the GP posterior of `k_gp_sweep4`, `k_gp_sweep` and `k_gp_small` against the posterior in "
             "extended precision (`tests/np_gp_truth.py`): per case cond(K), the oracle's own error, a NumPy restatement of the "
             "engine's formula and the engine's measured error (`tests/test_gpu_gp_truth.py`; DESIGN.md 6 (iv)).",
             "* `dispatch_matrix.md`: every instantiation the `sl_with_dim` lists of `sl_bellman.hip`, `sl_bellman4.hip`, "
             "`sl_succ.hip` and `sl_policy_solve.hip` compile - the test that reaches it or why none can "
             "(`tests/bellman_matrix.py`), the largest oracle and cross-kernel differences of the newly covered ones "
             "(`tests/test_gpu_bellman_matrix.py`) and the outcome of two numerically perturbed scratch builds.",
             "* `network_parity.md`: the twelve `k_nn_check_mfma<layers, d>` instantiations of `sl_nn.hip` with the test that "
             "reaches each, V, grad V and the sweep records against the network in extended precision "
             "(`tests/np_network_truth.py`, `tests/test_gpu_network_matrix.py`) per case, the device `sl_tanh` in ulp per "
             "segment, and the outcome of two numerically perturbed scratch builds.",
             "* `gp_sweep_matrix.md`: the 105 instantiations of `k_gp_small` (`sl_gp_small.hip`) and `k_gp_sweep` (`sl_gp.hip`) "
             "with the test that reaches each (`tests/gp_sweep_matrix.py`), the posterior of the newly covered ones against "
             "the long-double posterior in units of the oracle's own error, 4 / 12 / 16 against eight wavefronts bit for bit "
             "(`tests/test_gpu_gp_sweep_matrix.py`), wall times, and the outcome of two numerically perturbed scratch builds.",
             ""]
    for key in sorted(by_round):
        text.append("* %s: %s" % (key, ", ".join("`%s`" % n for n in by_round[key])))
    with open(os.path.join(P, "README.md"), "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text[:30]))


if __name__ == "__main__":
    main()
