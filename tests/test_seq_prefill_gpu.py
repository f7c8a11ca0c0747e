"""Episode prefill of the decoder-only baselines on the MI355X: `seq_steps` (vima_seq_decode_chunk), `seq_restart(history=)`
(vima_seq_decode_restart_history) and `seq_history_room`.

Models: syn.BaselineConfig(kind, 256, 2, heads, vocab_size=16, n_positions=...), B = 3, prompts from the ragged layout of
BASELINE_CASES["baseline_gato"] (one Lp, a different number of valid tokens per sample); Gato Q = 16, GPT Q = 1; 8 heads (D = 32), one Gato case
each at 16 heads (D = 16: the generic attention kernel) and 4 heads (D = 64). Gates: `_close` of tests/test_seq_ring_gpu.py (two routes of the same
sample); "bit for bit" is torch.equal. The bookkeeping is held against tests/seq_prefill_reference.py.

Observed max |delta| of the chunks against the 9 (GPT: 35) single steps on the linear cache (test 2; profiles/seq_prefill_pytest.txt): fp32 0.0,
bf16x3 0.0 (bit-identical), bf16 6.8e-4 (Gato), 7.7e-4 (GPT), 7.2e-4 (Gato, head dim 64) absolute at max |ref| of a few units."""
import ctypes
import functools

import pytest
import torch

from oracle.baseline_oracle import build_baseline_oracle
from oracle.cases import run_baseline
from tests import seq_prefill_reference as sp
from tests.gpu_common import bare_policy, loaded_policy, max_abs, ptr
from tests.test_seq_ring_gpu import _close, _cut, _cut_prompt, _data, _gate_oracle, _lp, _policy, _raw_prompt
from vima_amd import _lib
from vima_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
X3 = "bf16x3"
B = sp.B
E = 256
BASE_UNITS = [(0, 3), (3, 1), (4, 2), (6, 3)]


@functools.lru_cache(maxsize=None)
def _model(kind, heads, npos):
    cfg = syn.BaselineConfig(kind, E, 2, heads, vocab_size=16, n_positions=npos)
    return cfg, syn.make_baseline_state_dict(cfg, 5200 + heads + npos, head_gain=0.5)


def _prompt(pol, e):
    with torch.no_grad():
        t, m = pol.forward_prompt_assembly(syn.to_device(_raw_prompt(e), DEV))
    return t.contiguous().clone(), m.clone()


def _unit(pol, otok, atok, t, T):
    """batch steps t .. t + T - 1 from the streams: T = 1 through seq_step, longer through seq_steps -> [T, B, E]"""
    if T == 1:
        return pol.seq_step(otok[t].contiguous(), atok[t - 1] if t > 0 else None).unsqueeze(0)
    act = atok[t - 1:t + T - 1] if t > 0 else atok[0:T - 1]
    return pol.seq_steps(otok[t:t + T].contiguous(), act.contiguous())


def _forward_alone(ref, otok, atok, ts, b, pt, pm):
    """`forward` on the history of sample b alone: the env steps `ts` (indices into the streams) -> [len(ts), E]"""
    o = otok[ts, b:b + 1].contiguous()
    a = atok[ts[:-1], b:b + 1].contiguous() if len(ts) > 1 else None
    return ref.forward(o, a, pt[:, b:b + 1].contiguous(), pm[b:b + 1])[:, 0]


# ------------------------------------------------------------------------------------------ 1. T = 1 is the single step
@pytest.mark.parametrize("ring", [0, 1])
@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_one_step_chunk_is_the_single_step(kind, ring):
    cfg, sd = _model(kind, 8, _lp(kind) + 1 + sp.RING[kind])
    a, b = _policy(cfg, sd, "bf16", seq_ring=ring), _policy(cfg, sd, "bf16", seq_ring=ring)
    _, _, otok, atok = _data(a, 4)
    pt, pm = _prompt(a, 0)
    a.seq_prefill(pt, pm), b.seq_prefill(pt, pm)
    for t in range(4):
        want = a.seq_step(otok[t].contiguous(), atok[t - 1] if t else None)
        got = b.seq_steps(otok[t:t + 1].contiguous(), atok[t - 1:t].contiguous() if t else None)
        assert tuple(got.shape) == (1, B, E) and torch.equal(got[0], want), t
        assert a.steps_left().tolist() == b.steps_left().tolist()
        assert a.seq_history_room() == b.seq_history_room() == t + 1


def test_one_step_chunk_hits_the_graphs_of_the_single_step():
    """Four passes over the same 4 steps with static buffers: a key is captured the second time it is seen, so by the third pass every step replays;
    the fourth pass goes through seq_steps with T = 1, replays every step and captures nothing."""
    cfg, sd = _model("gato", 8, 192)
    pol = _policy(cfg, sd, "bf16", graphs=1)
    _, _, otok, atok = _data(pol, 4)
    pt, pm = _prompt(pol, 0)
    so, sa = torch.empty_like(otok[0]), torch.empty_like(atok[0])
    outs = torch.empty(4, 4, B, E, device=DEV)
    stats = []
    for p in range(4):
        pol.seq_prefill(pt, pm)
        for t in range(4):
            so.copy_(otok[t])
            if t:
                sa.copy_(atok[t - 1])
            if p < 3:
                out = pol.seq_step(so, sa if t else None)
            else:
                out = pol.seq_steps(so.unsqueeze(0), sa.unsqueeze(0) if t else None)[0]
            outs[p, t].copy_(out)
            del out
        torch.cuda.synchronize()
        stats.append(pol.graph_stats())
    print(f"[seq_prefill] graphs (replays, captures) after each pass: {stats}")
    assert stats[2][1] > 0 and stats[3][1] == stats[2][1] and stats[3][0] == stats[2][0] + 4, stats
    assert all(torch.equal(outs[p], outs[0]) for p in range(1, 4))


# ------------------------------------------------------------------------------------------ 2. chunks on the linear cache
@pytest.mark.parametrize("kind,heads,prec", [("gato", 8, "fp32"), ("gato", 8, "bf16"), ("gato", 8, X3), ("gpt", 8, "fp32"), ("gpt", 8, "bf16"), ("gpt", 8, X3),
                                             ("gato", 16, "fp32"), ("gato", 4, "bf16")])
def test_chunks_on_the_linear_cache(kind, heads, prec):
    """Units (0, 3), (3, 1), (4, 2), (6, 3): the first chunk starts at batch step 0 (no action row in its first slot). Gato reads >= 64 keys from the
    first unit on; GPT stays below 64 keys (the other branch of the attention launcher) through these units and then takes one chunk of 26 steps,
    rows 25 .. 76, whose keys cross 64 inside the chunk."""
    Q, Lp = sp.Q[kind], _lp(kind)
    units = BASE_UNITS + ([(9, 26)] if kind == "gpt" else [])
    steps = sum(T for _, T in units)
    npos = 192 if kind == "gato" else 80
    cfg, sd = _model(kind, heads, npos)
    pol, ref = _policy(cfg, sd, prec), _policy(cfg, sd, prec)
    _, _, otok, atok = _data(pol, steps)
    pt, pm = _prompt(pol, 0)
    book = sp.SeqBook(Lp, npos, Q, B, False)
    pol.seq_prefill(pt, pm)
    got = []
    for t, T in units:
        row, lq, _ = book.advance(T)
        if kind == "gato":
            assert row + lq >= 64
        elif T < 26:
            assert row + lq < 64
        else:
            assert row < 64 < row + lq
        got.append(_unit(pol, otok, atok, t, T))
        assert pol.steps_left().tolist() == book.steps_left() and pol.seq_history_room() == book.room()
    got = torch.cat(got)
    ref.seq_prefill(pt, pm)
    single = torch.cat([_unit(ref, otok, atok, t, 1) for t in range(steps)])
    worst = 0.0
    for b in range(B):
        full = _forward_alone(ref, otok, atok, list(range(steps)), b, pt, pm)
        for t in range(steps):
            _close(got[t, b], full[t], prec, (kind, "forward", b, t))
            _close(got[t, b], single[t, b], prec, (kind, "single steps", b, t))
        worst = max(worst, max_abs(got[:, b], single[:, b]))
    print(f"[seq_prefill] {kind} heads {heads} {prec}: chunks {units} against {steps} single steps: max |delta| {worst:.3e}")


# ------------------------------------------------------------------------------------------ 3. chunked ring rollout
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_chunked_ring_rollout(kind, prec):
    """The 26 steps with the staggered restarts of tests/seq_ring_reference.py, every third unit a chunk of two steps (tests/test_seq_prefill_build.py
    holds what the schedule contains): every (sample, episode) against `forward` alone on a ring-off policy, one late episode against the CPU
    oracle, steps_left against the restatement after every unit."""
    Q, Lp, R = sp.Q[kind], _lp(kind), sp.RING[kind]
    cfg, sd = _model(kind, 8, Lp + 1 + R)
    pol, ref = _policy(cfg, sd, prec, seq_ring=1), _policy(cfg, sd, prec, seq_ring=0)
    obs, acts, otok, atok = _data(pol, sp.STEPS)
    book = sp.SeqBook(Lp, Lp + 1 + R, Q, B, True)
    prompts = {}

    def prompt(e):
        if e not in prompts:
            prompts[e] = _prompt(pol, e)
        return prompts[e]

    number = [0] * B
    pt, pm = (x.clone() for x in prompt(0))
    episodes = {(b, 0): (pt[:, b:b + 1].clone(), pm[b:b + 1].clone(), 0) for b in range(B)}
    outs, lap, laps = [], 0, []
    pol.seq_prefill(pt, pm)
    for t, T in sp.units():
        flags = sp.restarts(t)
        if any(flags):
            for b in range(B):
                if flags[b]:
                    number[b] += 1
                    nt, nm = prompt(number[b])
                    pt[:, b], pm[b] = nt[:, b], nm[b]
                    episodes[(b, t)] = (nt[:, b:b + 1].clone(), nm[b:b + 1].clone(), number[b])
            pol.seq_restart(flags, pt, pm)
            book.restart(flags)
        row, _, _ = book.advance(T)
        lap += t == 0 or row == book.P0
        laps += [lap] * T
        outs.append(_unit(pol, otok, atok, t, T))
        assert pol.steps_left().tolist() == book.steps_left(), t
        assert pol.seq_history_room() == book.room(), t
    outs = torch.cat(outs)
    ends = sp.rr.episode_starts(sp.STEPS)
    assert set(ends) == set(episodes)
    wa = wr = 0.0
    for (b, t0), t1 in ends.items():
        ptok, pmask, _ = episodes[(b, t0)]
        act = atok[t0:t1 - 1, b:b + 1].contiguous() if t1 - t0 > 1 else None
        full = ref.forward(otok[t0:t1, b:b + 1].contiguous(), act, ptok, pmask)[:, 0]
        for t in range(t0, t1):
            a, r = _close(outs[t, b], full[t - t0], prec, ((b, t0), t))
            wa, wr = max(wa, a), max(wr, r)
    print(f"[seq_prefill] chunked ring {kind} {prec}: {len(ends)} episodes over {max(laps)} laps, worst max_abs {wa:.3e} max_rel {wr:.3e}")
    if prec == "fp32":   # the longest episode that begins in the latest lap that has one, on its raw inputs
        (b, t0), t1 = max(ends.items(), key=lambda kv: (laps[kv[0][1]], kv[1] - kv[0][1], -kv[0][0]))
        assert laps[t0] >= 3
        orc = build_baseline_oracle(cfg, sd)
        o, a = _cut(obs, acts, t0, t1, b)
        want = run_baseline(orc, _cut_prompt(_raw_prompt(episodes[(b, t0)][2]), b), o, a)["predicted"][:, 0]
        _gate_oracle(outs[t0:t1, b], want, f"seq_prefill {kind} sample {b} steps {t0}..{t1 - 1} (lap {laps[t0]}) vs oracle")


# ------------------------------------------------------------------------------------------ 4. refusals change nothing
def test_a_refused_linear_chunk_changes_nothing():
    cfg, sd = _model("gato", 8, 192)
    pol, ctl = _policy(cfg, sd, "bf16"), _policy(cfg, sd, "bf16")
    _, _, otok, atok = _data(pol, 10)
    pt, pm = _prompt(pol, 0)
    pol.seq_prefill(pt, pm), ctl.seq_prefill(pt, pm)
    for _ in range(2):
        with pytest.raises(IndexError, match="room for 9 more steps"):     # 38 + 10 * 17 - 1 = 207 > 192; (192 - 38 + 1) // 17 = 9
            _unit(pol, otok, atok, 0, 10)
    assert torch.equal(_unit(pol, otok, atok, 0, 3), _unit(ctl, otok, atok, 0, 3))
    with pytest.raises(IndexError, match="room for 6 more steps"):
        _unit(pol, otok, atok, 3, 7)
    assert torch.equal(_unit(pol, otok, atok, 3, 6), _unit(ctl, otok, atok, 3, 6))
    assert pol.steps_left().tolist() == [0] * B and pol.seq_history_room() == 9


def test_a_ring_chunk_refused_where_a_single_step_passes_changes_nothing():
    kind = "gato"
    Q, Lp, R = sp.Q[kind], _lp(kind), sp.RING[kind]
    cfg, sd = _model(kind, 8, Lp + 1 + R)
    pol, ctl = _policy(cfg, sd, "bf16", seq_ring=1), _policy(cfg, sd, "bf16", seq_ring=1)
    _, _, otok, atok = _data(pol, 12)
    pt, pm = _prompt(pol, 0)
    book = sp.SeqBook(Lp, Lp + 1 + R, Q, B, True)
    pol.seq_prefill(pt, pm), ctl.seq_prefill(pt, pm)
    t = 0
    while True:   # samples 0 and 1 are restarted before step 3: sample 2 is the oldest; stop where one more step fits but a chunk of two does not
        if t == 3:
            for p in (pol, ctl):
                p.seq_restart([True, True, False], pt, pm)
            book.restart([True, True, False])
        if t >= 3:
            book.plan(1)
            try:
                book.plan(2)
            except IndexError as e:
                assert "sample 2" in str(e)
                break
        book.advance(1)
        assert torch.equal(_unit(pol, otok, atok, t, 1), _unit(ctl, otok, atok, t, 1))
        t += 1
        assert t < 11
    left = pol.steps_left().tolist()
    assert left == book.steps_left() and left[2] >= 1
    with pytest.raises(IndexError, match="sample 2"):
        _unit(pol, otok, atok, t, 2)
    assert pol.steps_left().tolist() == left and pol.seq_history_room() == book.room()
    book.advance(1)
    assert torch.equal(_unit(pol, otok, atok, t, 1), _unit(ctl, otok, atok, t, 1))
    assert pol.steps_left().tolist() == book.steps_left() == ctl.steps_left().tolist()


def test_a_refused_install_changes_nothing_and_the_other_refusals():
    kind = "gato"
    cfg, sd = _model(kind, 8, 192)
    pol, ctl = _policy(cfg, sd, "bf16"), _policy(cfg, sd, "bf16")
    _, _, otok, atok = _data(pol, 8)
    pt, pm = _prompt(pol, 0)
    nt, nm = _prompt(pol, 1)
    pol.seq_prefill(pt, pm), ctl.seq_prefill(pt, pm)
    for t in range(3):
        _unit(pol, otok, atok, t, 1), _unit(ctl, otok, atok, t, 1)
    assert pol.seq_history_room() == 3
    with pytest.raises(IndexError, match="room for 3"):
        pol.seq_restart([False, True, False], nt, nm, history=(otok[4:8, 1:2].contiguous(), atok[4:7, 1:2].contiguous()))
    assert pol.seq_history_room() == 3
    assert torch.equal(_unit(pol, otok, atok, 3, 1), _unit(ctl, otok, atok, 3, 1))       # sample 1 is still in its old episode: its action row was read
    # the Python surface
    with pytest.raises(AssertionError, match="action_token"):
        pol.seq_steps(otok[4:6].contiguous())
    with pytest.raises(AssertionError, match="action_token"):
        pol.seq_steps(otok[4:6].contiguous(), atok[4:5].contiguous())                     # [T - 1, B, E] after the first step
    with pytest.raises(AssertionError, match="obs_token"):
        pol.seq_steps(otok[4].contiguous(), atok[3:4].contiguous())
    with pytest.raises(AssertionError, match="history"):
        pol.seq_restart([False, True, False], nt, nm, history=(otok[4:6].contiguous(), atok[4:5].contiguous()))          # B columns instead of n_r
    # the C entries
    lib, h = pol._lib, pol._handle
    o2, a2 = otok[4:6].contiguous(), atok[3:5].contiguous()
    out = torch.empty(2, B, E, device=DEV)
    room = ctypes.c_int32(0)
    o1, a1 = o2[:, 1:2].contiguous(), a2[:1, 1:2].contiguous()
    flags = torch.tensor([0, 1, 0], dtype=torch.uint8)

    def chunk(hh, step=4, act=a2):
        return lib.vima_seq_decode_chunk(hh, ptr(o2), ptr(act), step, 2, B, ptr(out), None)

    def install(hh):
        return lib.vima_seq_decode_restart_history(hh, ctypes.c_void_p(flags.data_ptr()), B, ptr(nt), nt.stride(1), nt.stride(0), ptr(nm), nt.shape[0],
                                                   ptr(o1), ptr(a1), 2, None, None)

    def msg():
        return lib.vima_last_error().decode()

    assert chunk(h, act=None) != 0 and "action tokens" in msg()
    assert chunk(h, step=5) != 0 and "does not continue the episode state" in msg()
    fcfg = syn.BaselineConfig("flamingo", E, 1, 8, xattn_n_heads=8)
    fl = _policy(fcfg, syn.make_baseline_state_dict(fcfg, 6), "bf16")
    vcfg = syn.config("2M")
    vp = loaded_policy(vcfg, syn.make_state_dict(vcfg, 0), "bf16")
    for hh, why in ((fl._handle, "GPT / GATO"), (vp._handle, "baseline policies")):
        assert chunk(hh) != 0 and why in msg()
        assert install(hh) != 0 and why in msg()
        assert lib.vima_seq_history_room(hh, ctypes.byref(room)) != 0 and why in msg()
    pol.set_option("decode_ring", 1)
    for call in (lambda: chunk(h), lambda: install(h), lambda: lib.vima_seq_history_room(h, ctypes.byref(room))):
        assert call() != 0 and "decode_ring" in msg()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 5. install on the linear cache
def _with_sample(x, b, row):
    x = x.clone()
    x[b] = row
    return x


@pytest.mark.parametrize("prec", ["fp32", "bf16", X3])
@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_install_on_the_linear_cache(kind, prec):
    """Batch A takes 6 steps; sample 1's replacement episode (its own prompt, stream steps 10 .. 12 of sample 1) is installed as 3 steps of history,
    then 3 more batch steps in which sample 1 continues that episode (stream steps 13 .. 15)."""
    Q, Lp = sp.Q[kind], _lp(kind)
    npos = 192 if kind == "gato" else 80
    cfg, sd = _model(kind, 8, npos)
    pol, ctl, zero = (_policy(cfg, sd, prec) for _ in range(3))
    _, _, otok, atok = _data(pol, 16)
    pt, pm = _prompt(pol, 0)
    nt, nm = _prompt(pol, 1)
    qt, qm = pt.clone(), pm.clone()
    qt[:, 1], qm[1] = nt[:, 1], nm[1]
    book = sp.SeqBook(Lp, npos, Q, B, False)
    for p in (pol, ctl, zero):
        p.seq_prefill(pt, pm)
        for t in range(6):
            _unit(p, otok, atok, t, 1)
    for _ in range(6):
        book.advance(1)
    flags = [False, True, False]
    assert pol.seq_history_room() == book.room() == 6
    pred = pol.seq_restart(flags, qt, qm, history=(otok[10:13, 1:2].contiguous(), atok[10:12, 1:2].contiguous()))
    book.install(flags, 3)
    assert tuple(pred.shape) == (3, 1, E) and pol.seq_history_room() == book.room() == 6
    assert ctl.seq_restart(flags, qt, qm) is None
    assert tuple(zero.seq_restart(flags, qt, qm, history=(otok[0:0, 1:2].contiguous(), None)).shape) == (0, 1, E)      # T = 0 IS seq_restart
    later = []
    for t in range(6, 9):
        o, a = _with_sample(otok[t], 1, otok[t + 7, 1]), _with_sample(atok[t - 1], 1, atok[t + 6, 1])
        got, want, z = (p.seq_step(o.contiguous(), a.contiguous()) for p in (pol, ctl, zero))
        book.advance(1)
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]), t       # the other samples: untouched by the install
        assert torch.equal(z, want), t
        later.append(got[1])
        assert pol.steps_left().tolist() == book.steps_left() and pol.seq_history_room() == book.room()
    full = _forward_alone(ctl, otok, atok, list(range(10, 16)), 1, qt, qm)
    for s in range(3):
        _close(pred[s, 0], full[s], prec, (kind, "teacher-forced", s))
        _close(later[s], full[3 + s], prec, (kind, "after the install", s))


def _launches(pol, fn):
    pol.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    n = sum(v["launches"] for v in pol.prof_read().values())
    pol.prof_enable(False)
    return n


def test_install_launch_counts():
    """An install takes the same launches for one and for two flagged samples; T = 0 takes those of seq_restart."""
    cfg, sd = _model("gato", 8, 192)
    pol = _policy(cfg, sd, "bf16")
    _, _, otok, atok = _data(pol, 8)
    pt, pm = _prompt(pol, 0)
    nt, nm = _prompt(pol, 1)
    n = {}
    for who in ([1], [1, 2]):
        flags = [b in who for b in range(B)]
        for T in (None, 0, 3):
            pol.seq_prefill(pt, pm)
            for t in range(3):
                _unit(pol, otok, atok, t, 1)
            hist = None if T is None else (otok[4:4 + T, who].contiguous(), atok[4:4 + T - 1, who].contiguous() if T > 1 else None)
            n[(len(who), T)] = _launches(pol, lambda: pol.seq_restart(flags, nt, nm, history=hist))
    print(f"[seq_prefill] launches of seq_restart (flagged samples, T): {n}")
    assert n[(1, 3)] == n[(2, 3)] > 0 and n[(1, 0)] == n[(1, None)] == n[(2, 0)] == n[(2, None)] > 0, n


# ------------------------------------------------------------------------------------------ 6. install on the ring
RING_CASE = {"gato": (6, 8, 10), "gpt": (4, 6, 8)}     # every sample restarted before step tr; step tw wraps; the install comes before step ti


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [2, 3], ids=["behind-the-wrap", "straddling-the-wrap"])
@pytest.mark.parametrize("kind", ["gato", "gpt"])
def test_install_on_the_ring(kind, T, prec):
    """Single steps; all samples restarted before step tr so that the ring wraps legally at step tw; before step ti = tw + 2 samples 0 and 2 are plainly
    restarted and sample 1 takes T steps of history (stream steps 20 ..): T = 2 lies in the slots of steps tw, tw + 1 behind the wrap, T = 3 also in
    the slot of step tw - 1 at the ring's end. The control restarts sample 1 plainly right before batch step ti - T. Then sample 1, the oldest,
    steps on until its steps_left entry is 0 and the next step is refused naming it."""
    Q, Lp, R = sp.Q[kind], _lp(kind), sp.RING[kind]
    tr, tw, ti = RING_CASE[kind]
    cfg, sd = _model(kind, 8, Lp + 1 + R)
    pol, ctl, ref = _policy(cfg, sd, prec, seq_ring=1), _policy(cfg, sd, prec, seq_ring=1), _policy(cfg, sd, prec, seq_ring=0)
    _, _, otok, atok = _data(pol, 40)
    p0, p1, p2, p3 = (_prompt(pol, e) for e in range(4))
    book, cbook = sp.SeqBook(Lp, Lp + 1 + R, Q, B, True), sp.SeqBook(Lp, Lp + 1 + R, Q, B, True)
    pol.seq_prefill(*p0), ctl.seq_prefill(*p0)
    one = [False, True, False]
    q2t, q2m = p1[0].clone(), p1[1].clone()
    q2t[:, 1], q2m[1] = p2[0][:, 1], p2[1][1]
    for t in range(ti):
        if t == tr:
            for p, bk in ((pol, book), (ctl, cbook)):
                p.seq_restart([True] * B, *p1)
                bk.restart([True] * B)
        if t == ti - T:
            ctl.seq_restart(one, q2t, q2m)
            cbook.restart(one)
        row, lq, adv = book.advance(1)
        assert cbook.advance(1) == (row, lq, adv) and (t > 0 and (adv > lq or row == book.P0)) == (t == tw)
        _unit(pol, otok, atok, t, 1), _unit(ctl, otok, atok, t, 1)
    others = [True, False, True]
    q3t, q3m = q2t.clone(), q2m.clone()
    for b in (0, 2):
        q3t[:, b], q3m[b] = p3[0][:, b], p3[1][b]
    for p, bk in ((pol, book), (ctl, cbook)):
        p.seq_restart(others, q3t, q3m)
        bk.restart(others)
    rowmap = book.rowmap(T)
    assert len(rowmap) == Lp + T * (Q + 1) and rowmap != list(range(len(rowmap))) and len(set(rowmap)) == len(rowmap)
    hist_rows = rowmap[Lp + 1:]
    wrapped_first = book.slots[tw][0]
    assert (min(hist_rows) >= wrapped_first and max(hist_rows) < book.slots[tw - 1][0]) if T == 2 else max(hist_rows) >= book.slots[tw - 1][0] > wrapped_first
    assert pol.seq_history_room() == book.room() >= T
    hs = list(range(20, 20 + T))
    pred = pol.seq_restart(one, q3t, q3m, history=(otok[hs, 1:2].contiguous(), atok[hs[:-1], 1:2].contiguous()))
    book.install(one, T)
    assert pol.steps_left().tolist() == book.steps_left() and pol.steps_left()[1].item() == ctl.steps_left()[1].item() == cbook.steps_left()[1]
    assert pol.seq_history_room() == book.room()
    mine, t, k = [], ti, 0
    while True:
        o, a = _with_sample(otok[t], 1, otok[20 + T + k, 1]).contiguous(), _with_sample(atok[t - 1], 1, atok[20 + T + k - 1, 1]).contiguous()
        if book.steps_left()[1] == 0:
            with pytest.raises(IndexError, match="sample 1"):
                pol.seq_step(o, a)
            assert pol.steps_left().tolist() == book.steps_left()
            break
        got = pol.seq_step(o, a)
        book.advance(1)
        if k < 2:        # the unflagged samples against the control, whose sample 1 runs another episode
            want = ctl.seq_step(o, a)
            assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]), t
        mine.append(got[1])
        assert pol.steps_left().tolist() == book.steps_left()
        t, k = t + 1, k + 1
        assert t < 40 - 1 and 20 + T + k < 40
    assert k >= 2
    full = _forward_alone(ref, otok, atok, list(range(20, 20 + T + k)), 1, q3t, q3m)
    for s in range(T):
        _close(pred[s, 0], full[s], prec, (kind, T, "teacher-forced", s))
    for s in range(k):
        _close(mine[s], full[T + s], prec, (kind, T, "after the install", s))


# ------------------------------------------------------------------------------------------ 7. graphs
def test_chunk_and_install_between_graphed_steps():
    """Per pass: prefill, 3 steps, a chunk of 2, 2 steps, an install of 2 steps for sample 1, 2 steps -- static buffers. Eager against graphs = 1, four
    passes each: a key is captured the second time it is seen; the last pass replays all 7 single steps and captures nothing, although a chunk and an
    install ran eager in between."""
    cfg, sd = _model("gato", 8, 192)
    results = []
    for graphs in (0, 1):
        pol = _policy(cfg, sd, "bf16", graphs=graphs)
        _, _, otok, atok = _data(pol, 12)
        pt, pm = _prompt(pol, 0)
        nt, nm = _prompt(pol, 1)
        so, sa = torch.empty_like(otok[0]), torch.empty_like(atok[0])
        outs = torch.zeros(4, 9, B, E, device=DEV)
        stats = []

        def step(p, t):
            so.copy_(otok[t])
            if t:
                sa.copy_(atok[t - 1])
            out = pol.seq_step(so, sa if t else None)
            outs[p, t].copy_(out)
            del out

        for p in range(4):
            pol.seq_prefill(pt, pm)
            for t in range(3):
                step(p, t)
            outs[p, 3:5].copy_(_unit(pol, otok, atok, 3, 2))
            for t in (5, 6):
                step(p, t)
            pol.seq_restart([False, True, False], nt, nm, history=(otok[10:12, 1:2].contiguous(), atok[10:11, 1:2].contiguous()))
            for t in (7, 8):
                step(p, t)
            torch.cuda.synchronize()
            stats.append(pol.graph_stats())
        results.append((outs, stats))
    (eager, _), (graphed, stats) = results
    print(f"[seq_prefill] graphs (replays, captures) after each pass: {stats}")
    assert torch.equal(eager, graphed)
    assert stats[3][1] == stats[2][1] > 0 and stats[3][0] == stats[2][0] + 7, stats


# ------------------------------------------------------------------------------------------ 8. kernels per element
CANARY = 0xA5


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("Ew", [256, 320])
@pytest.mark.parametrize("has_act", [0, 1])
@pytest.mark.parametrize("Q", [1, 16])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_seq_embed_chunk_per_element(T, Q, has_act, Ew, prec):
    pol = bare_policy(prec)
    g = torch.Generator().manual_seed(100 * T + 10 * Q + has_act + Ew)
    Ln = T * (Q + 1) - (1 - has_act)
    row0, n_pos = 5, 5 + Ln + 3
    obs = torch.randn(T, B, Q, Ew, generator=g)
    n_act = T if has_act else T - 1
    act = torch.randn(max(n_act, 1), B, Ew, generator=g)
    table = torch.randn(n_pos, Ew, generator=g)
    posbase = torch.tensor([5, n_pos - 1, 0, -77], dtype=torch.int32)       # sample 1 reaches the clamp at the table's last row; entry 3: not a sample
    fresh = torch.tensor([1, 0, 1, CANARY], dtype=torch.uint8)
    cmask = torch.full((B + 1, n_pos), CANARY, dtype=torch.uint8)
    want = torch.empty(B, Ln, Ew)
    wmask, wpos = cmask.clone(), posbase.clone()
    for b in range(B):
        skip = int(has_act and fresh[b].item())
        for l in range(Ln):
            j = l + (1 - has_act)
            u, s = divmod(j, Q + 1)
            tok = torch.zeros(Ew) if (l == 0 and skip) else (act[u - (1 - has_act), b] if s == 0 else obs[u, b, s - 1])
            pid = int(posbase[b]) + l - (skip if l > 0 else 0)
            want[b, l] = tok + table[min(max(pid, 0), n_pos - 1)]
            wmask[b, row0 + l] = 0 if (l == 0 and skip) else 1
        wpos[b] = int(posbase[b]) + Ln - skip
    assert int(posbase[1]) + Ln - 1 >= n_pos - 1
    wfresh = torch.tensor([0, 0, 0, CANARY], dtype=torch.uint8)
    d = dict(obs=obs.to(DEV), act=act.to(DEV), table=table.to(DEV), cmask=cmask.to(DEV), pos=posbase.to(DEV), fresh=fresh.to(DEV),
             x=torch.full((B, Ln, Ew), float("nan"), device=DEV), xT=torch.full((B, Ln, Ew), float("nan"), device=DEV))
    _lib.check(pol._lib.vima_op_seq_embed_chunk(pol._handle, ptr(d["obs"]), ptr(d["act"]) if n_act else None, ptr(d["table"]), n_pos, row0, T, B, Q, has_act,
                                                Ew, ptr(d["x"]), ptr(d["xT"]), ptr(d["cmask"]), ptr(d["pos"]), ptr(d["fresh"]), pol._stream()))
    torch.cuda.synchronize()
    assert torch.equal(d["x"].cpu(), want)
    assert torch.equal(d["xT"].cpu(), want.to(torch.bfloat16).float() if prec == "bf16" else want)
    assert torch.equal(d["cmask"].cpu(), wmask) and torch.equal(d["pos"].cpu(), wpos) and torch.equal(d["fresh"].cpu(), wfresh)


def test_seq_embed_chunk_refusals():
    pol = bare_policy("bf16")
    f = torch.zeros(64 * 256, device=DEV)
    u8 = torch.zeros(64, dtype=torch.uint8, device=DEV)
    i32 = torch.zeros(4, dtype=torch.int32, device=DEV)
    call = lambda n_pos, row0, T, act: pol._lib.vima_op_seq_embed_chunk(pol._handle, ptr(f), act, ptr(f), n_pos, row0, T, 1, 4, 1, 256, ptr(f), None, ptr(u8),
                                                                        ptr(i32), ptr(u8), pol._stream())
    assert call(12, 3, 2, ptr(f)) != 0 and "seq_embed_chunk" in pol._lib.vima_last_error().decode()       # 3 + 10 > 12
    assert call(32, 3, 2, None) != 0                                                                       # action rows without act_tok
    assert call(32, 3, 2, ptr(f)) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("seed", [0, 1])
def test_seq_history_install_per_element(seed):
    pol = bare_policy("bf16")
    g = torch.Generator().manual_seed(40 + seed)
    n_s, n_pos, Lp, Q, T = 5, 300 if seed else 64, 6, 4, 3
    L = Lp + T * (Q + 1)
    lo, hi = Lp + 1, n_pos - 7
    lst = torch.tensor([3, 1], dtype=torch.int32)
    hist = (torch.randperm(hi - lo, generator=g)[:L - Lp - 1] + lo).tolist()        # distinct rows inside [lo, hi), in no order
    rowmap = torch.tensor(list(range(Lp + 1)) + hist, dtype=torch.int32)
    mask = (torch.rand(2, L, generator=g) > 0.3).to(torch.uint8) * 3                # any non-zero byte is "valid"
    cmask = torch.full((n_s, n_pos), CANARY, dtype=torch.uint8)
    pos = torch.full((n_s,), -5, dtype=torch.int32)
    fresh = torch.full((n_s,), CANARY, dtype=torch.uint8)
    wm, wp, wf = cmask.clone(), pos.clone(), fresh.clone()
    for r, b in enumerate(lst.tolist()):
        wm[b, lo:hi] = 0
        wm[b, rowmap.long()] = (mask[r] != 0).to(torch.uint8)
        wp[b], wf[b] = int((mask[r] != 0).sum()), 0
    d = [x.to(DEV) for x in (mask, lst, rowmap, cmask, pos, fresh)]
    _lib.check(pol._lib.vima_op_seq_history_install(pol._handle, ptr(d[0]), ptr(d[1]), ptr(d[2]), 2, L, lo, hi, n_pos, ptr(d[3]), ptr(d[4]), ptr(d[5]),
                                                    pol._stream()))
    torch.cuda.synchronize()
    assert torch.equal(d[3].cpu(), wm) and torch.equal(d[4].cpu(), wp) and torch.equal(d[5].cpu(), wf)
    assert pol._lib.vima_op_seq_history_install(pol._handle, ptr(d[0]), ptr(d[1]), ptr(d[2]), 2, L, lo, n_pos + 1, n_pos, ptr(d[3]), ptr(d[4]), ptr(d[5]),
                                                pol._stream()) != 0
