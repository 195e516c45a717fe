"""What an opt-in rule of the actor (SearchOptions.of: playout_cap, leaf_symmetry, forced_playouts, gumbel, fpu_reduction; aux_targets;
policy_surprise; visit_reduction) costs it.

Runs the headline shape of bench.py (9x9 Go, 4096 games, 200 simulations, 8 leaves per round, 10 x 128 network, fp32-class
evaluator) twice on the same build, with the same staggered openings and the same number of untimed and timed rounds: once with the
rule off -- the yardstick -- and once with it on.  Prints one JSON line per run and one with the ratios.  The searches of the two runs
differ (a rule changes what is selected or evaluated), so the rates are those of two different, equally long workloads, not of one
workload timed twice.  Except under the playout cap every timed round is bracketed by events, so besides moves/s and sims/s each run
reports the mean time of the select kernel, of expand / backup + end of move and of the forward.  What each option adds:

playout_cap (--value FAST,FULL_PROB, default 40,0.25; 400 timed rounds after 300): samples/s (every recorded sample) and full samples/s
  (the samples a learner is handed: all of them with the cap off, the full-search ones with it on).  Samples are counted when their
  game is harvested, and a timed window of a few hundred rounds is shorter than a game, so the sample and game rates of a run depend on
  how many games happen to end inside the window; moves/s and sims/s do not.  full_moves_per_s = moves/s x the full fraction of the
  harvested samples is the rate at which full-search samples are PRODUCED, whenever their games end.
leaf_symmetry (--value random or an op 0..7): the ops of the last round's rows.  Select draws the ops and permutes the planes, expand /
  backup gathers the priors back, the forward sees nothing but other boards.
forced_playouts (--value K, default 2, KataGo's): select runs the forced test in front of every descent, the end of a move prunes the
  target.  Both runs log the last search of every slot (one log row per slot), so the on run can compare, every `--sample-every` rounds,
  each slot's target row with the unpruned policy of the same search: the share of searches whose target pruning changed.
gumbel (--value M, default 16): select chooses the considered action in front of every descent, the end of a move forms the base row,
  a* and pi'.  `--parent DIR` names a built checkout of the parent commit: `python bench.py --gpus 1 --steps S --warmup W` -- the
  headline workload, the mode off -- then first runs `--pairs` times in each tree, in fresh processes, alternating (parent, child, ...;
  `--child-first` swaps the order inside a pair).  Printed: moves/s of every run in the order they ran, the parent's spread (max - min
  over its runs), and child - parent pair by pair.  The off path may be slower than the parent by no more than that spread.

fpu_reduction (--value R or R_TREE,R_ROOT, default 0.2,0.1, KataGo's): select takes one more wave reduction per tree level, in the kernel
  that holds the rule.  The tree changes shape (deeper, narrower), so each run also reports, per simulation, the tree levels walked
  (node_visits), the hint prefetches and the hint hits: a change of the select time is the reduction's or the descents'.  A third run
  builds the actor with the rule on and turns it off before the first round: the plain search in the kernel that holds the rule, which
  an engine keeps launching once it has enabled it (`off_after_on_over_off`).  `--parent DIR` as under gumbel.

aux_targets (no value): the end of a move stores the root value, the end of a game the owner boards, every harvest (`--harvest-every`) writes
  and clones the three extra outputs.  The searches of the two runs are the same here: nothing but the extra outputs differs.

policy_surprise (--value FRAC or FRAC,1 to include fast moves; default 0.5): the end of a move takes 2 A float64 logs and one wave
  reduction, every harvest sums each game's surprises and writes two more outputs.  The searches of the two runs are the same.
  `--replay-adds ROWS` (default 0 = skip) then times DeviceReplay.add_samples against add_samples(weights=) on ROWS random 9x9 rows
  with weights around 1: a warm-up, then `--windows` windows of 10 calls each, microseconds per call with the spread between windows.

visit_reduction (--value THRESHOLD,LOOKBACK,MIN_SIMULATIONS,MIN_WEIGHT, default 0,2,20,0.25): the start of a move reads the slot's ring of
  root values, the end of a search pushes onto it, every harvest writes the base weights and the weights.  The bench network has
  random weights and its root values stay near 0, so the default threshold is 0: a move is reduced as soon as one side has led, by
  however little, in the last two searches, and by the share of the lead.  Each run reports the share of moves started with a reduced
  budget (reduced_moves / moves), simulations per move and the mean base weight harvested.  `--parent DIR` as under gumbel.

    python tools/search_option_rate.py --option {playout_cap,leaf_symmetry,forced_playouts,gumbel,fpu_reduction,aux_targets,policy_surprise,visit_reduction} [--value ...] [--steps 300] [--preroll 200]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from alpha_zero_amd.core.network import AlphaZeroNet  # noqa: E402
from alpha_zero_amd.core.pipeline import SelfPlayActor  # noqa: E402
from engine_util import random_openings  # noqa: E402


class Extra:
    """What an option adds to the run body: by default nothing.  `on`: the option's value in this run (None in the off run)."""
    steps, preroll, phases, actor_kw = 300, 200, True, {}
    ratios = ("on_over_off", ("moves_per_s", "sims_per_s", "select_us", "backup_endmove_us", "forward_us"), 4)

    def __init__(self, args, act, on):
        self.args, self.act, self.on = args, act, on

    def after_round(self, i):
        pass

    def after_harvest(self, z, games):
        pass

    def row(self, cnt, dt):
        return {}


class PlayoutCap(Extra):
    steps, preroll, phases = 400, 300, False
    ratios = ("cap_on_over_cap_off", ("moves_per_s", "full_moves_per_s", "samples_per_s", "full_samples_per_s", "games_per_s"), 3)
    samples = full = games = 0

    @staticmethod
    def parse(text):
        fast, prob = (text or "40,0.25").split(",")
        return int(fast), float(prob)

    def after_harvest(self, z, games):
        self.samples, self.games, self.full = self.samples + int(z.shape[0]), self.games + len(games), self.full + int(self.act.last_harvest_full.sum().item())

    def row(self, cnt, dt):
        samples, full = self.samples, self.full
        return dict(samples_per_s=round(samples / dt, 1), full_samples_per_s=round(full / dt, 1), full_fraction=round(full / max(1, samples), 4),
                    full_moves_per_s=round(cnt["moves"] / dt * full / max(1, samples), 1), games_per_s=round(self.games / dt, 2),
                    sims_per_move=round(cnt["sims"] / max(1, cnt["moves"]), 1))


class LeafSymmetry(Extra):
    @staticmethod
    def parse(text):
        return "random" if text in (None, "random") else int(text)

    def row(self, cnt, dt):
        e = self.act.engine
        return dict(ops_of_the_last_round=np.bincount(e.leaf_symmetries().cpu().numpy()[e.valid.cpu().numpy().astype(bool)], minlength=8).tolist())


class ForcedPlayouts(Extra):
    actor_kw = dict(engine_kw=dict(log_moves=True, log_capacity=1))  # one log row per slot: its last finished search
    searched = changed = 0

    @staticmethod
    def parse(text):
        return float(text or 2.0)

    def after_round(self, i):
        if self.on and (i + 1) % self.args.sample_every == 0:  # (device tensors; the two sums are read after the clock stops)
            e = self.act.engine
            pi, target = e.read_searches()[0], e.target_policies()
            done = target.sum(1) > 0
            self.searched = self.searched + done.sum()
            self.changed = self.changed + (done & (target != pi).any(1)).sum()

    def row(self, cnt, dt):
        searched, changed = int(self.searched), int(self.changed)
        return dict(searches_sampled=searched, targets_changed_by_pruning=changed, share_changed=round(changed / searched, 4) if searched else None)


class Gumbel(Extra):
    @staticmethod
    def parse(text):
        return int(text or 16)


class FpuReduction(Extra):
    @staticmethod
    def parse(text):
        r = tuple(float(v) for v in (text or "0.2,0.1").split(","))
        return r if len(r) == 2 else r[0]

    def row(self, cnt, dt):
        sims = max(1, cnt["sims"])
        return dict(node_visits_per_sim=round(cnt["node_visits"] / sims, 3), hint_prefetches_per_sim=round(cnt["hint_prefetches"] / sims, 3),
                    hint_hits_per_sim=round(cnt["hint_hits"] / sims, 3))


class AuxTargets(Extra):
    samples = 0

    @staticmethod
    def parse(text):
        return True

    def after_harvest(self, z, games):
        self.samples += int(z.shape[0])
        assert not self.on or self.act.last_harvest_aux.root_q.shape == z.shape

    def row(self, cnt, dt):
        return dict(samples_harvested=self.samples)


class PolicySurprise(Extra):
    samples, weight = 0, 0.0

    @staticmethod
    def parse(text):
        frac, _, fast = (text or "0.5").partition(",")
        return (float(frac), fast.strip() not in ("", "0"))

    def after_harvest(self, z, games):
        self.samples += int(z.shape[0])
        if self.on:
            assert self.act.last_harvest_weight.shape == z.shape
            self.weight = self.weight + self.act.last_harvest_weight.sum()  # (a device scalar; read after the clock stops)

    def row(self, cnt, dt):
        return dict(samples_harvested=self.samples, weight_harvested=round(float(self.weight), 1))


class VisitReduction(Extra):
    samples, base = 0, 0.0

    @staticmethod
    def parse(text):
        t, look, sims, w = (text or "0,2,20,0.25").split(",")
        return float(t), int(look), int(sims), float(w)

    def after_harvest(self, z, games):
        self.samples += int(z.shape[0])
        if self.on:
            assert self.act.last_harvest_base.shape == self.act.last_harvest_weight.shape == z.shape
            self.base = self.base + self.act.last_harvest_base.sum()  # (a device scalar; read after the clock stops)

    def row(self, cnt, dt):
        moves = max(1, cnt["moves"])
        return dict(reduced_share=round(cnt.get("reduced_moves", 0) / moves, 4), sims_per_move=round(cnt["sims"] / moves, 1),
                    samples_harvested=self.samples, mean_base=round(float(self.base) / self.samples, 4) if self.on and self.samples else None)


def replay_add_rate(args):
    """add_samples against add_samples(weights=) on the same `--replay-adds` rows: microseconds per call, per window of 10 calls."""
    from alpha_zero_amd.core.replay import DeviceReplay

    n, rows, dev = args.board, args.replay_adds, torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    st = (torch.rand(rows, 17, n, n, generator=g) > 0.6).to(torch.int8).to(dev)
    pi = torch.rand(rows, n * n + 1, generator=g).to(dev)
    z = torch.randint(-1, 2, (rows,), generator=g).float().to(dev)
    w = (torch.rand(rows, generator=g) * 2).to(dev)  # mean 1: about as many rows written as the plain add writes
    rep = DeviceReplay(1 << 18, np.random.RandomState(1), n, n * n + 1, device=dev)
    out = {}
    for name, kw in (("add_samples", {}), ("add_samples_weighted", dict(weights=w))):
        for _ in range(5):
            rep.add_samples(st, pi, z, **kw)
        wins = []
        for _ in range(args.windows):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(10):
                rep.add_samples(st, pi, z, **kw)
            torch.cuda.synchronize(dev)
            wins.append((time.perf_counter() - t0) / 10 * 1e6)
        out[name] = dict(us_per_call=[round(v, 1) for v in wins], mean=round(float(np.mean(wins)), 1), spread=round(max(wins) - min(wins), 1))
    print(json.dumps(dict(replay_adds=dict(rows=rows, **out))), flush=True)


OPTIONS = dict(playout_cap=PlayoutCap, leaf_symmetry=LeafSymmetry, forced_playouts=ForcedPlayouts, gumbel=Gumbel, fpu_reduction=FpuReduction,
               aux_targets=AuxTargets, policy_surprise=PolicySurprise, visit_reduction=VisitReduction)


def bench_line(tree, steps, warmup):
    """The result line of one `bench.py` run in `tree` (a process of its own)."""
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline",
                          "--no-companions", "--no-fresh-tree"], cwd=tree, capture_output=True, text=True, check=True, timeout=600).stdout
    for row in reversed(out.strip().split("\n")):
        if row.startswith("{") and '"value"' in row:
            return json.loads(row)
    raise SystemExit("no result line from bench.py in " + tree)


def off_against_parent(args):
    runs = []
    order = [("child", ROOT), ("parent", args.parent)] if args.child_first else [("parent", args.parent), ("child", ROOT)]
    for _ in range(args.pairs):
        for who, tree in order:
            line = bench_line(tree, args.bench_steps, args.bench_warmup)
            runs.append(dict(build=who, moves_per_s=line["value"], serial_step_ms=line.get("serial_step_ms")))
            print(json.dumps(runs[-1]), flush=True)
    par = [r["moves_per_s"] for r in runs if r["build"] == "parent"]
    chi = [r["moves_per_s"] for r in runs if r["build"] == "child"]
    spread = max(par) - min(par)
    print(json.dumps(dict(off_against_parent=dict(parent=par, child=chi, parent_spread=round(spread, 2),
                                                  child_minus_parent=[round(c - p, 2) for c, p in zip(chi, par)],
                                                  mean_child_minus_parent=round(float(np.mean(chi) - np.mean(par)), 2),
                                                  within_parent_spread=bool(np.mean(chi) >= np.mean(par) - spread)))), flush=True)


def run(args, on, then_off=False):
    """One run with the option at `on` (None = off): the actor, the staggered openings of bench.py (mixed game phases from the first
    round), the untimed rounds, the timed rounds, the result row.  then_off (fpu_reduction): the actor is built with the rule on and the
    rule is turned off before the first round."""
    n, dev, kind = args.board, torch.device("cuda"), OPTIONS[args.option]
    torch.manual_seed(1)
    net = AlphaZeroNet((17, n, n), n * n + 1, args.blocks, args.filters, args.filters)
    act = SelfPlayActor(net, game="go", board_size=n, num_games=args.games, num_simulations=args.sims, num_parallel=args.parallel,
                        warm_up_steps=16, resign_threshold=-1.0, seed=1, device=dev, net_dtype=torch.float32, **{args.option: on}, **kind.actor_kw)
    if then_off:
        act.engine.set_fpu_reduction(None)
    extra = kind(args, act, on)
    rng = np.random.Generator(np.random.PCG64(1234))
    random_openings(act.engine, rng.integers(0, args.stagger + 1, size=args.games), rng)
    for i in range(args.preroll):
        act.run_round()
        if (i + 1) % args.harvest_every == 0:
            act.harvest_tensors()
    act.harvest_tensors()
    act.counters(reset=True)
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.steps)] if kind.phases else None
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(args.steps):
        act.run_round(evs[i] if evs else None)
        if (i + 1) % args.harvest_every == 0:
            _, _, z, games = act.harvest_tensors()
            extra.after_harvest(z, games)
        extra.after_round(i)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    cnt = act.counters()
    res = {args.option: "off after on" if then_off else list(on) if isinstance(on, tuple) else on, "rounds": args.steps, "seconds": round(dt, 3),
           "moves_per_s": round(cnt["moves"] / dt, 1), "sims_per_s": round(cnt["sims"] / dt, 1)}
    if evs:
        phase = lambda a: round(float(np.mean([ev[a].elapsed_time(ev[a + 1]) for ev in evs])) * 1e3, 1)  # noqa: E731  (microseconds)
        res.update(backup_endmove_us=phase(0), select_us=phase(1), forward_us=phase(2))
    res.update(extra.row(cnt, dt))
    if evs:
        res["range_events"] = act.range_events
    res["evaluator"] = act.evaluator_path
    act.engine.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--option", required=True, choices=sorted(OPTIONS))
    ap.add_argument("--value", default=None, help="the option's value in the on run: FAST,FULL_PROB | random or an op 0..7 | k | m | r or r_tree,r_root")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--preroll", type=int, default=None)
    ap.add_argument("--harvest-every", type=int, default=50)
    ap.add_argument("--sample-every", type=int, default=25, help="forced_playouts: rounds between two looks at the target rows")
    ap.add_argument("--stagger", type=int, default=60)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--parallel", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--parent", default=None, help="gumbel, fpu_reduction, visit_reduction: a built checkout of the parent commit: bench.py runs there and here, alternating")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--child-first", action="store_true")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--no-on", action="store_true", help="only the off path against the parent")
    ap.add_argument("--replay-adds", type=int, default=0, help="policy_surprise: rows of one replay add to time, plain against weighted (0 = skip)")
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    kind = OPTIONS[args.option]
    args.steps, args.preroll = args.steps or kind.steps, kind.preroll if args.preroll is None else args.preroll
    if args.parent:
        off_against_parent(args)
    if args.replay_adds:
        replay_add_rate(args)
    if args.no_on:
        return
    off = run(args, None)
    print(json.dumps(off), flush=True)
    on = run(args, kind.parse(args.value))
    print(json.dumps(on), flush=True)
    label, keys, digits = kind.ratios
    print(json.dumps({label: {key: round(on[key] / off[key], digits) if off[key] else None for key in keys}}))
    if args.option == "fpu_reduction":
        after = run(args, kind.parse(args.value), then_off=True)
        print(json.dumps(after), flush=True)
        print(json.dumps({"off_after_on_over_off": {key: round(after[key] / off[key], digits) if off[key] else None for key in keys}}))


if __name__ == "__main__":
    main()
