"""The `episodes` case group of scripts/stage_fold_equivalence.py: every episode entry point of the C ABI (vima_decode_step / _chunk / _restart /
_restart_history / _history_room / _steps_left / _fork / _snapshot / _restore and their vima_seq_* twins) on small shapes, and their host-side
refusals. episode_cases(Rec, DEV) -> {name: (time limit, function)}; the child-process machinery and the comparison stay in
stage_fold_equivalence.py, which registers the group:

    python scripts/stage_fold_equivalence.py PARENT_LIB NEW_LIB --only episodes > profiles/episode_entry_equivalence.txt

Beyond the output hashes and launch logs of the other groups, a case records `values` (history_room, steps_left, graph_stats) and `refusals`
(the return code and the vima_last_error() text of every refused call): both libraries must agree on them byte for byte."""
import ctypes
import dataclasses

B, Q = 4, 2


def episode_cases(Rec, DEV):
    import torch
    from vima_amd import _lib
    from vima_testing import synthetic as syn

    # ------------------------------------------------------------------------------------------------ helpers
    def rand(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)

    def refused(rec, name, call):
        """a call the library must refuse: its exception type (= the return code's class) and message"""
        try:
            call()
        except Exception as e:   # noqa: BLE001 - whatever the binding raises is what is compared
            rec.out["refusals"].append([name, type(e).__name__, str(e)])
        else:
            rec.out["refusals"].append([name, "NOT REFUSED", ""])

    def raw(rec, pol, name, fn, *args):
        """the C entry itself, behind no Python check: return code and vima_last_error()"""
        code = getattr(pol._lib, fn)(pol._handle, *args)
        rec.out["refusals"].append([name + ": " + fn, int(code), pol._lib.vima_last_error().decode("utf-8", "replace") if code else ""])
        torch.cuda.synchronize()

    def vima_policy(prec, npos=512, **opts):
        from vima_amd.policy import VIMAPolicy
        cfg = dataclasses.replace(syn.config("2M"), n_positions=npos)
        pol = VIMAPolicy(**cfg.ctor_kwargs(), n_positions=npos, precision=prec, device=DEV)
        pol.load_state_dict(syn.make_state_dict(cfg, 3, head_gain=0.5), strict=True)
        for k, v in opts.items():
            pol.set_option(k, v)
        return pol

    def tokens_per_obs(kind):
        return syn.BaselineConfig(kind, 256, 2, 8).obs_tokens

    def seq_policy(kind, npos=512, prec="bf16", **opts):
        from vima_amd.baselines import build_baseline
        cfg = syn.BaselineConfig(kind, 256, 2, 8, xattn_n_heads=8 if kind == "flamingo" else 0, vocab_size=16, n_positions=npos)
        pol = build_baseline(cfg, precision=prec, device=DEV)
        pol.load_state_dict(syn.make_baseline_state_dict(cfg, 41, head_gain=0.5), strict=True)
        for k, v in opts.items():
            pol.set_option(k, v)
        return pol

    class Feed:
        """random tokens of a batch: prompts per (sample, episode), obs / actions per step"""

        def __init__(self, E, Lp, nb=B, q=Q, seed=0):
            self.E, self.Lp, self.B, self.Q, self.seed = E, Lp, nb, q, seed
            self.prompt = rand(seed + 1, Lp, nb, E)
            self.pmask = torch.ones(nb, Lp, dtype=torch.bool, device=DEV)
            for b in range(nb):
                self.pmask[b, Lp - b % 3:] = False               # ragged: 0, 1 or 2 padded tokens
            self.omask = torch.ones(nb, q, dtype=torch.bool, device=DEV)

        def obs(self, t, n=1):
            return rand(self.seed + 100 + t, n, self.B, self.Q, self.E)

        def act(self, t, n=1):
            return rand(self.seed + 500 + t, n, self.B, self.E)

        def new_prompts(self, flags, t):
            fresh = rand(self.seed + 900 + t, self.Lp, self.B, self.E)
            for b, f in enumerate(flags):
                if f:
                    self.prompt[:, b] = fresh[:, b]

    # ------------------------------------------------------------------------------------------------ XAttnGPT (VIMA)
    def vima_episode(prec, Lp, hm, npos=512, ring=0, steps=12):
        pol = vima_policy(prec, npos, kv_headmajor=hm, decode_ring=ring)
        rec, f = Rec(pol), Feed(pol.embed_dim, Lp)
        rec.out["engaged"]["options"] = dict(precision=prec, Lp=Lp, kv_headmajor=hm, decode_ring=ring, n_positions=npos)
        t = 0

        def step(tag=""):
            nonlocal t
            left = pol.steps_left().tolist() if t else []
            if ring and t and 0 in left:                         # the samples out of ring rows start a new episode
                flags = [n == 0 for n in left]
                f.new_prompts(flags, t)
                pol.restart_samples(flags, f.prompt, f.pmask)
                rec.step("restart (out of steps) in front of step %d" % t)
            out = pol.forward_step(f.obs(t)[0], f.omask, f.act(t)[0] if t else None, f.prompt, f.pmask, t)
            rec.tensor("step %d%s" % (t, tag), out)
            rec.step("step %d%s" % (t, tag))
            rec.out["values"]["after step %d" % t] = dict(history_room=pol.history_room(), steps_left=pol.steps_left().tolist())
            t += 1

        step(), step()
        rec.tensor("chunk of 3 at step 2", pol.forward_steps(f.obs(t, 3), f.omask.expand(3, B, Q), f.act(t, 3), f.prompt, f.pmask, t))
        rec.step("chunk of 3")
        t += 3
        pol.restart_samples([0, 0, 0, 0], f.prompt, f.pmask)
        rec.step("restart of none")
        f.new_prompts([1, 0, 1, 0], t)
        pol.restart_samples([1, 0, 1, 0], f.prompt, f.pmask)
        rec.step("restart of 2")
        step(" after restart")
        f.new_prompts([0, 1, 0, 0], t)
        hist = (rand(71, 2, 1, Q, f.E), torch.ones(2, 1, Q, dtype=torch.bool, device=DEV), rand(72, 1, 1, f.E))
        rec.tensor("restart with history T=2", pol.restart_samples([0, 1, 0, 0], f.prompt, f.pmask, history=hist))
        rec.step("restart with history")
        step(" after history")
        f.prompt, f.pmask = pol.fork_samples([0, 0, 2, 2], f.prompt, f.pmask)
        rec.step("fork")
        step(" after fork")
        with_p = pol.snapshot_samples([0, 3], f.prompt, f.pmask, with_prompt=True)
        rec.step("snapshot with prompt")
        without = pol.snapshot_samples([1], f.prompt, f.pmask, with_prompt=False)
        rec.step("snapshot without prompt")
        for i, s in enumerate(with_p + without):
            rec.tensor("snapshot payload %d (%d steps)" % (i, s.steps), s.payload)
        step(" after snapshot")
        f.prompt, f.pmask = pol.restore_samples([2, 1], [with_p[0], without[0]], f.prompt, f.pmask)
        rec.step("restore")
        step(" after restore")
        while t < steps:
            step()
        rec.out["engaged"]["steps taken"] = t
        return rec

    def vima_graphs(ring):
        """the step loop under option graphs (profiling off: it disables the graph path): three passes over the same tensors"""
        pol = vima_policy("bf16", 24 if ring else 512, decode_ring=ring, graphs=1)
        rec, f = Rec(pol), Feed(pol.embed_dim, 8)
        pol.prof_enable(False)
        obs, act = [f.obs(t)[0] for t in range(7)], [f.act(t)[0] for t in range(7)]
        out = []
        for lap in range(3):
            for t in range(7):
                out.append(pol.forward_step(obs[t], f.omask, act[t] if t else None, f.prompt, f.pmask, t).clone())
            rec.out["values"]["graph_stats after pass %d" % lap] = list(pol.graph_stats())
        rec.tensor("all steps", torch.stack(out))
        return rec

    # ------------------------------------------------------------------------------------------------ decoder-only (GPT / Gato), Flamingo
    def seq_episode(kind, ring, steps=20):
        q = tokens_per_obs(kind)
        Lp, nb = 6, 3
        pol = seq_policy(kind, Lp + 1 + 8 * (q + 1) if ring else 512, seq_ring=ring)
        rec, f = Rec(pol), Feed(pol.embed_dim, Lp, nb, q)
        rec.out["engaged"]["options"] = dict(kind=kind, seq_ring=ring, Q=q)
        t = 0

        def step(tag=""):
            nonlocal t
            left = pol.steps_left().tolist()
            if ring and 0 in left:
                flags = [n == 0 for n in left]
                f.new_prompts(flags, t)
                pol.seq_restart(flags, f.prompt, f.pmask)
                rec.step("seq_restart (out of steps) in front of step %d" % t)
            out = pol.seq_step(f.obs(t)[0], f.act(t)[0] if t else None)
            rec.tensor("seq_step %d%s" % (t, tag), out)
            rec.step("seq_step %d%s" % (t, tag))
            rec.out["values"]["after step %d" % t] = dict(history_room=pol.seq_history_room(), steps_left=pol.steps_left().tolist())
            t += 1

        pol.seq_prefill(f.prompt, f.pmask)
        rec.step("seq_prefill")
        step(), step(), step()
        rec.tensor("seq_steps(3)", pol.seq_steps(f.obs(t, 3), f.act(t, 3)))
        rec.step("seq_steps(3)")
        t += 3
        pol.seq_restart([0, 0, 0], f.prompt, f.pmask)
        rec.step("seq_restart of none")
        f.new_prompts([1, 0, 1], t)
        pol.seq_restart([1, 0, 1], f.prompt, f.pmask)
        rec.step("seq_restart of 2")
        step(" after restart")
        f.new_prompts([0, 1, 0], t)
        rec.tensor("seq_restart with history T=2", pol.seq_restart([0, 1, 0], f.prompt, f.pmask, history=(rand(73, 2, 1, q, f.E), rand(74, 1, 1, f.E))))
        rec.step("seq_restart with history")
        step(" after history")
        pol.seq_fork([0, 0, 2])
        rec.step("seq_fork")
        step(" after fork")
        snaps = pol.seq_snapshot([0, 2])
        rec.step("seq_snapshot")
        for i, s in enumerate(snaps):
            rec.tensor("snapshot payload %d (%d steps)" % (i, s.steps), s.payload)
        step(" after snapshot")
        pol.seq_restore([1], [snaps[0]])
        rec.step("seq_restore")
        step(" after restore")
        while t < steps:
            step()
        return rec

    def flamingo_episode():
        pol = seq_policy("flamingo")
        rec, f = Rec(pol), Feed(pol.embed_dim, 8, 3, tokens_per_obs("flamingo"))
        for t in range(2):
            rec.tensor("forward_step %d" % t, pol.forward_step(f.obs(t)[0], f.act(t)[0] if t else None, f.prompt, f.pmask, t))
            rec.step("forward_step %d" % t)
        f.new_prompts([1, 0, 1], 2)
        pol.restart_samples([1, 0, 1], f.prompt, f.pmask)
        rec.step("restart")
        rec.tensor("forward_step 2", pol.forward_step(f.obs(2)[0], f.act(2)[0], f.prompt, f.pmask, 2))
        rec.step("forward_step 2")
        rec.out["values"]["end"] = dict(history_room=pol.history_room(), steps_left=pol.steps_left().tolist())
        return rec

    # ------------------------------------------------------------------------------------------------ refusals: all on the host, nothing is launched
    def entry_args(pol, nb, q, Lp, null=None):
        """every episode entry with well-formed arguments for a batch of nb samples (device pointers into one zeroed buffer that is larger than
        anything the entry could touch, host arrays for the host arguments); null = (entry, position): that pointer argument is NULL"""
        E, st = pol.embed_dim, pol._stream()
        buf = torch.zeros(1 << 21, dtype=torch.float32, device=DEV)
        d = ctypes.c_void_p(buf.data_ptr())
        flags = (ctypes.c_uint8 * nb)(*([1] * nb))
        i32 = (ctypes.c_int32 * nb)(*range(nb))
        one = ctypes.c_int32(0)
        infos = (_lib.VimaEpisodeSnapshotInfo * nb)()
        ptrs = (ctypes.c_void_p * nb)(*[buf.data_ptr() + (b << 20) for b in range(nb)])
        caps = (ctypes.c_int64 * nb)(*([1 << 20] * nb))
        hf, hi, hp, hc, hinfo = (ctypes.cast(x, ctypes.c_void_p) for x in (flags, i32, ptrs, caps, infos))
        sb, sl = E, nb * E
        A = {
            "vima_decode_step": [d, d, d, 1, nb, q, d, sb, sl, d, Lp, d, st],
            "vima_decode_chunk": [d, d, d, 1, 2, nb, q, d, sb, sl, d, Lp, d, st],
            "vima_decode_restart": [hf, nb, d, sb, sl, d, Lp, st],
            "vima_decode_restart_history": [hf, nb, d, sb, sl, d, Lp, d, d, d, 1, d, st],
            "vima_decode_history_room": [ctypes.byref(one)],
            "vima_decode_steps_left": [nb, i32],
            "vima_decode_fork": [i32, nb, st],
            "vima_decode_snapshot_size": [i32, nb, 1, hinfo],
            "vima_decode_snapshot": [i32, nb, 1, hp, hc, hinfo, st],
            "vima_decode_restore": [i32, nb, hp, hinfo, st],
            "vima_seq_decode_step": [d, d, 1, nb, d, st],
            "vima_seq_decode_chunk": [d, d, 1, 2, nb, d, st],
            "vima_seq_decode_restart": [hf, nb, d, sb, sl, d, Lp, st],
            "vima_seq_decode_restart_history": [hf, nb, d, sb, sl, d, Lp, d, d, 1, d, st],
            "vima_seq_history_room": [ctypes.byref(one)],
            "vima_seq_decode_fork": [i32, nb, st],
            "vima_seq_decode_snapshot_size": [i32, nb, 1, hinfo],
            "vima_seq_decode_snapshot": [i32, nb, 1, hp, hc, hinfo, st],
            "vima_seq_decode_restore": [i32, nb, hp, hinfo, st],
        }
        if null:
            A = {null[0]: list(A[null[0]])}
            A[null[0]][null[1]] = None
        return A, (buf, flags, i32, one, infos, ptrs, caps)

    # (entry, position of a required pointer argument among those behind the handle)
    # (a NULL the entry does not check for would be refused all the same: the step / chunk arguments carry a stale step number)
    NULLS = [("vima_decode_step", 2), ("vima_decode_chunk", 2), ("vima_decode_restart", 0), ("vima_decode_restart", 2),
             ("vima_decode_restart", 5), ("vima_decode_restart_history", 0), ("vima_decode_restart_history", 7), ("vima_decode_restart_history", 8),
             ("vima_decode_history_room", 0), ("vima_decode_steps_left", 1), ("vima_decode_fork", 0), ("vima_decode_snapshot_size", 0),
             ("vima_decode_snapshot_size", 3), ("vima_decode_snapshot", 3), ("vima_decode_snapshot", 4), ("vima_decode_restore", 0),
             ("vima_decode_restore", 2), ("vima_decode_restore", 3)]
    SEQ_NULLS = [("vima_seq_decode_step", 0), ("vima_seq_decode_step", 1), ("vima_seq_decode_step", 4), ("vima_seq_decode_chunk", 1),
                 ("vima_seq_decode_restart", 0), ("vima_seq_decode_restart", 2), ("vima_seq_decode_restart", 5), ("vima_seq_decode_restart_history", 0),
                 ("vima_seq_decode_restart_history", 7), ("vima_seq_history_room", 0), ("vima_seq_decode_fork", 0), ("vima_seq_decode_snapshot_size", 0),
                 ("vima_seq_decode_snapshot", 3), ("vima_seq_decode_restore", 0), ("vima_seq_decode_restore", 2), ("vima_seq_decode_restore", 3)]

    def sweep(rec, pol, what, nb, q, Lp, family):
        A, keep = entry_args(pol, nb, q, Lp)
        for fn, args in A.items():
            if fn.startswith("vima_seq") == (family == "seq"):
                raw(rec, pol, what, fn, *args)

    def run_two(pol, f):
        for t in range(2):
            pol.forward_step(f.obs(t)[0], f.omask, f.act(t)[0] if t else None, f.prompt, f.pmask, t)

    def vima_refusals():
        nb, Lp = 3, 8
        pol = vima_policy("bf16")
        rec, f = Rec(pol), Feed(pol.embed_dim, Lp, nb)
        sweep(rec, pol, "no running batch", nb, Q, Lp, "decode")
        sweep(rec, pol, "the other family's handle", nb, Q, Lp, "seq")
        raw(rec, pol, "the other family's handle", "vima_seq_prefill", ctypes.c_void_p(f.prompt.data_ptr()), f.E, nb * f.E,
            ctypes.c_void_p(f.pmask.data_ptr()), nb, Lp, pol._stream())
        run_two(pol, f)
        sweep(rec, pol, "the other family's handle, while its own batch runs", nb, Q, Lp, "seq")
        for null in NULLS:
            A, keep = entry_args(pol, nb, Q, Lp, null)
            stale = null in (("vima_seq_decode_step", 1), ("vima_seq_decode_chunk", 1))   # seq action tokens: checked behind the continuity check
            raw(rec, pol, ("null action tokens behind a stale step (the continuity refusal comes first)" if stale else "null argument %d" % null[1]),
                null[0], *A[null[0]])
        refused(rec, "step out of order", lambda: pol.forward_step(f.obs(5)[0], f.omask, f.act(5)[0], f.prompt, f.pmask, 5))
        refused(rec, "step repeated", lambda: pol.forward_step(f.obs(1)[0], f.omask, f.act(1)[0], f.prompt, f.pmask, 1))
        f2 = Feed(f.E, Lp, 2)
        refused(rec, "step with the wrong B", lambda: pol.forward_step(f2.obs(2)[0], f2.omask, f2.act(2)[0], f2.prompt, f2.pmask, 2))
        refused(rec, "chunk with the wrong B", lambda: pol.forward_steps(f2.obs(2, 2), f2.omask.expand(2, 2, Q), f2.act(2, 2), f2.prompt, f2.pmask, 2))
        f6 = Feed(f.E, 6, nb)
        refused(rec, "step with the wrong Lp", lambda: pol.forward_step(f6.obs(2)[0], f6.omask, f6.act(2)[0], f6.prompt, f6.pmask, 2))
        refused(rec, "restart with the wrong B", lambda: pol.restart_samples([1, 0], f2.prompt, f2.pmask))
        refused(rec, "restart with the wrong Lp", lambda: pol.restart_samples([1, 0, 1], f6.prompt, f6.pmask))
        hist3 = (rand(75, 3, 1, Q, f.E), torch.ones(3, 1, Q, dtype=torch.bool, device=DEV), rand(76, 2, 1, f.E))
        refused(rec, "restart history with the wrong B", lambda: pol.restart_samples([1, 0], f2.prompt, f2.pmask, history=hist3[:1] + hist3[1:]))
        refused(rec, "history longer than the room", lambda: pol.restart_samples([0, 1, 0], f.prompt, f.pmask, history=hist3))
        refused(rec, "fork with the wrong B", lambda: pol.fork_samples([0, 0], f2.prompt, f2.pmask))
        refused(rec, "fork chain", lambda: pol.fork_samples([1, 2, 2], f.prompt, f.pmask))
        refused(rec, "snapshot of a sample outside the batch", lambda: pol.snapshot_samples([3], f.prompt, f.pmask))
        # a snapshot of 4 steps into a batch that has taken 2
        other = vima_policy("bf16")
        for t in range(4):
            other.forward_step(f.obs(t)[0], f.omask, f.act(t)[0] if t else None, f.prompt, f.pmask, t)
        snap = other.snapshot_samples([1], f.prompt, f.pmask)
        refused(rec, "restore beyond the room", lambda: pol.restore_samples([0], snap, f.prompt, f.pmask))
        refused(rec, "restore into a slot outside the batch", lambda: pol.restore_samples([3], snap, f.prompt, f.pmask))
        rec.out["values"]["the running batch is untouched"] = dict(history_room=pol.history_room(), steps_left=pol.steps_left().tolist())
        rec.tensor("step 2 after the refusals", pol.forward_step(f.obs(2)[0], f.omask, f.act(2)[0], f.prompt, f.pmask, 2))
        # chunks that do not fit: linear, ring (longer than the ring; over a sample's age)
        for ring in (0, 1):
            small = vima_policy("bf16", 24, decode_ring=ring)
            run_two(small, f)
            for T in (7, 9):
                refused(rec, "chunk of %d at step 2, n_positions 24, decode_ring %d" % (T, ring),
                        lambda: small.forward_steps(f.obs(2, T), f.omask.expand(T, nb, Q), f.act(2, T), f.prompt, f.pmask, 2))
            for t in range(2, 9):
                refused(rec, "step %d, n_positions 24, decode_ring %d, nobody restarted" % (t, ring),
                        lambda: small.forward_step(f.obs(t)[0], f.omask, f.act(t)[0], f.prompt, f.pmask, t))
            rec.out["values"]["n_positions 24, decode_ring %d" % ring] = dict(history_room=small.history_room(), steps_left=small.steps_left().tolist())
        rec.step("all")
        return rec

    def seq_refusals(kind):
        nb, Lp = 3, 6
        q = tokens_per_obs(kind)
        pol = seq_policy(kind, Lp + 1 + 8 * (q + 1))
        rec, f = Rec(pol), Feed(pol.embed_dim, Lp, nb, q)
        sweep(rec, pol, "no running batch", nb, q, Lp, "seq")
        sweep(rec, pol, "the other family's handle", nb, q, Lp, "decode")
        pol.seq_prefill(f.prompt, f.pmask)
        pol.seq_step(f.obs(0)[0])
        pol.seq_step(f.obs(1)[0], f.act(1)[0])
        sweep(rec, pol, "the other family's handle, while its own batch runs", nb, q, Lp, "decode")
        for null in SEQ_NULLS:
            A, keep = entry_args(pol, nb, q, Lp, null)
            stale = null in (("vima_seq_decode_step", 1), ("vima_seq_decode_chunk", 1))   # seq action tokens: checked behind the continuity check
            raw(rec, pol, ("null action tokens behind a stale step (the continuity refusal comes first)" if stale else "null argument %d" % null[1]),
                null[0], *A[null[0]])
        A, keep = entry_args(pol, nb, q, Lp)
        raw(rec, pol, "step out of order", "vima_seq_decode_step", *(A["vima_seq_decode_step"][:2] + [5] + A["vima_seq_decode_step"][3:]))
        raw(rec, pol, "wrong B", "vima_seq_decode_step", *(A["vima_seq_decode_step"][:2] + [2, 2] + A["vima_seq_decode_step"][4:]))
        f2, f5 = Feed(f.E, Lp, 2, q), Feed(f.E, 5, nb, q)
        refused(rec, "seq_restart with the wrong B", lambda: pol.seq_restart([1, 0], f2.prompt, f2.pmask))
        refused(rec, "seq_restart with the wrong Lp", lambda: pol.seq_restart([1, 0, 1], f5.prompt, f5.pmask))
        refused(rec, "history longer than the room", lambda: pol.seq_restart([0, 1, 0], f.prompt, f.pmask, history=(rand(77, 3, 1, q, f.E), rand(78, 2, 1, f.E))))
        refused(rec, "history with the wrong Lp", lambda: pol.seq_restart([0, 1, 0], f5.prompt, f5.pmask, history=(rand(77, 2, 1, q, f.E), rand(78, 1, 1, f.E))))
        refused(rec, "seq_fork swap", lambda: pol.seq_fork([1, 0, 2]))
        refused(rec, "chunk that does not fit", lambda: pol.seq_steps(f.obs(2, 7), f.act(2, 7)))
        other = seq_policy(kind, Lp + 1 + 8 * (q + 1))
        other.seq_prefill(f.prompt, f.pmask)
        for t in range(4):
            other.seq_step(f.obs(t)[0], f.act(t)[0] if t else None)
        snap = other.seq_snapshot([1])
        refused(rec, "restore beyond the room", lambda: pol.seq_restore([0], snap))
        rec.out["values"]["the running batch is untouched"] = dict(history_room=pol.seq_history_room(), steps_left=pol.steps_left().tolist())
        rec.tensor("seq_step 2 after the refusals", pol.seq_step(f.obs(2)[0], f.act(2)[0]))
        ringed = seq_policy(kind, Lp + 1 + 8 * (q + 1), seq_ring=1)
        ringed.seq_prefill(f.prompt, f.pmask)
        ringed.seq_step(f.obs(0)[0])
        for T in (7, 9):
            refused(rec, "chunk of %d under seq_ring" % T, lambda: ringed.seq_steps(f.obs(1, T), f.act(1, T)))
        ringed.set_option("decode_ring", 1)
        refused(rec, "decode_ring on a decoder-only handle", lambda: ringed.seq_prefill(f.prompt, f.pmask))
        rec.step("all")
        return rec

    cases = {}
    for Lp in (40, 8):
        for hm in (1, 0):
            cases["episodes vima bf16 B=4 Lp=%d kv_headmajor=%d" % (Lp, hm)] = (180, lambda Lp=Lp, hm=hm: vima_episode("bf16", Lp, hm))
    cases["episodes vima fp32 B=4 Lp=8"] = (180, lambda: vima_episode("fp32", 8, 1))
    cases["episodes vima bf16 decode_ring n_positions=24 (the ring wraps twice)"] = (180, lambda: vima_episode("bf16", 8, 1, npos=24, ring=1, steps=24))
    cases["episodes vima bf16 graphs"] = (180, lambda: vima_graphs(0))
    cases["episodes vima bf16 graphs decode_ring"] = (180, lambda: vima_graphs(1))
    for kind in ("gpt", "gato"):
        for ring in (0, 1):
            cases["episodes %s seq_ring=%d" % (kind, ring)] = (180, lambda k=kind, r=ring: seq_episode(k, r))
    cases["episodes flamingo"] = (180, flamingo_episode)
    cases["episodes refusals vima"] = (240, vima_refusals)
    cases["episodes refusals gpt"] = (240, lambda: seq_refusals("gpt"))
    cases["episodes refusals gato"] = (240, lambda: seq_refusals("gato"))
    return cases
