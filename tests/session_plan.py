"""Planner of the long decode sessions (a plain module of the suite, not a conftest): `plan(kind, seed)` -> the list of ops one session
runs, every parameter concrete, with the lengths each op must leave behind.  Pure Python / numpy; nothing from mustafar_amd is imported:
the length rules below are an independent statement of the documented ones, and tests/session_util.py asserts the hook's
compressed_length, kv_seq_len and both Window.len against them after every op.

    * the trigger is due when (L - residual_length - C) % 256 == 0 and window >= 256;
    * a trigger point may only be the last row of a several-token call;
    * accept lowers L and the window by the rejected rows.

Ops (dicts; every op carries "L", "C", "W" = the lengths after it, "fired", "holes_compressed", "full_table", and "extents" = the entries
of the extent table in use where the table is cut to 2):

    step         decode_fused, one token ("lse"; "defer": defer_trigger=True)
    multi        decode_multi ("n_q", "mask": none | row | causal | tree, "parents" of a tree, "lse", "poison": per sequence the new
                 rows that are rejected later and carry poison)
    accept       closes the multi / multi_split before it: "rejected", or "keep" [B][n_keep] with "n_q"; "new_holes": per sequence the
                 live rows that stay in the cache although the sequence rejected them ("defer" as above)
    split        decode_split, one token ("frozen": "s" shared | "p" per-sequence | "sp" both)
    multi_split  decode_multi_split ("frozen", "n_q", "mask", "parents", "poison")
    run_triggers run_triggers() over all layers of the session ("pool": prepare_triggers() first, its result handed over)

A hole is a row that a sequence rejected and that stays in the cache (the padding of accept(keep=) where a sequence accepted less than
the longest), or a left-padding row of sequence 1 ("pad" of the header): from its birth on every call carries a mask with finfo.min on it.
decode_split refuses a mask next to a shared entry, so a `split` op has a shared entry only while no hole exists; afterwards the shared
entry is read by `multi_split` with n_q = 1.

The random choices are steered (never dropped) so that every plan meets the conditions tests/test_session_plan_host.py asserts."""
import numpy as np

R = 32               # residual_length
BLOCK = 256          # tokens of one trigger
B = 2                # sequences
HKV = 2              # kv heads
F_SHARED = 128       # tokens of the shared frozen entry
F_SEQ = 192          # tokens of the per-sequence frozen entry
TRIGGERS = 4         # a session ends once it has crossed this many
STARTS = (250, 300)  # prefill rows: nothing compressed (the first trigger creates the cache) / 256 compressed
PAD = 7              # left-padding rows of sequence 1 in the seeds that have them

# kind -> head_dim, q heads per kv head, layers, MustafarConfig keywords, whether the extent table is cut to 2 entries, whether the cache kind
# takes split ops (tests/test_gpu_shared_segment.SPLIT_KINDS: tuple at 64, ext64, arena at 128) and which helper kind builds its frozen
# entries (an ExtentCache64 holds whole 256-token blocks, so the 128 and 192 frozen tokens of the ext64 kinds arrive as reference-layout
# lists), whether a trigger can be deferred (arena and extent caches), the sparsities
KINDS = {
    "list128":         dict(head_dim=128, groups=4, layers=1, cfg=dict(), small_table=None, split=None, defer=False),
    "arena_inplace":   dict(head_dim=128, groups=4, layers=1, cfg=dict(arena=True, extents=False), small_table=None, split="arena", defer=True),
    "arena_ext":       dict(head_dim=128, groups=4, layers=2, cfg=dict(arena=True), small_table="arena", split="arena", defer=True),
    "arena_ext_tiles": dict(head_dim=128, groups=4, layers=1, cfg=dict(arena=True, key_rows=False), small_table="arena", split="arena",
                            defer=True),
    "arena_g2":        dict(head_dim=128, groups=2, layers=1, cfg=dict(arena=True), small_table=None, split="arena", defer=True),
    "list64":          dict(head_dim=64, groups=4, layers=1, cfg=dict(), small_table=None, split="tuple", defer=False),
    "ext64":           dict(head_dim=64, groups=4, layers=2, cfg=dict(hd64_extents=True), small_table="ext64", split="tuple", defer=True),
    "ext64_uneven":    dict(head_dim=64, groups=8, layers=1, cfg=dict(hd64_extents=True), small_table=None, split="tuple", defer=True,
                            k_sparsity=0.5, v_sparsity=0.8),
}
for _k in KINDS.values():
    _k.setdefault("k_sparsity", 0.7)
    _k.setdefault("v_sparsity", 0.7)

# seed bit 0: the start (250 / 300 rows); bit 1: left padding of sequence 1.  Two seeds per kind, every combination on either head dim
SEEDS = {
    "list128": (2, 5), "arena_inplace": (1, 6), "arena_ext": (0, 7), "arena_ext_tiles": (3, 4),
    "arena_g2": (2, 9), "list64": (0, 3), "ext64": (6, 1), "ext64_uneven": (5, 10),
}
SESSIONS = [(k, s) for k, seeds in SEEDS.items() for s in seeds]


def header(kind, seed):
    """What a session starts from: prefill rows, left padding of sequence 1."""
    return dict(start=STARTS[seed & 1], pad=PAD if seed & 2 else 0)


def trigger_due(L, C, W):
    return (L - R - C) % BLOCK == 0 and W >= BLOCK


class _Planner:
    def __init__(self, kind, seed):
        self.kind, self.k = kind, KINDS[kind]
        self.rng = np.random.default_rng([sorted(KINDS).index(kind), seed])
        h = header(kind, seed)
        self.L = h["start"]
        self.C = max(0, (self.L - R) // BLOCK * BLOCK)
        self.W = self.L - self.C
        self.holes = [set(), set(range(h["pad"]))]
        self.extents = 0                      # entries of the extent table in use (kinds whose table is cut to 2)
        self.triggers = 0
        self.ops = []
        self.per = 64 // self.k["groups"]     # tokens of one library call
        self.unequal_done = False

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def any_hole(self):
        return any(self.holes)

    def point(self):
        """kv_seq_len at the next trigger point."""
        return self.C + R + BLOCK

    def rem(self):
        return self.point() - self.L

    def split_ok(self):
        # decode_split asks the live call for an LSE, which a window-only call at head_dim 128 does not have
        return self.k["split"] is not None and (self.C > 0 or self.k["head_dim"] == 64)

    def emit(self, op, **kw):
        op = dict(op=op, **kw)
        op.update(L=self.L, C=self.C, W=self.W)
        op.setdefault("fired", False)
        op.setdefault("holes_compressed", 0)
        op.setdefault("full_table", False)
        op["extents"] = self.extents if self.k["small_table"] else None      # entries of the extent table in use behind the base
        self.ops.append(op)
        return op

    def close(self, defer=False):
        """The trigger rule after the rows of an op are counted -> the fields that describe what happened."""
        if not trigger_due(self.L, self.C, self.W):
            return dict(due=False)
        if defer:
            return dict(due=True, defer=True)
        return dict(due=True, **self.fire())

    def fire(self):
        lo, hi = self.C, self.C + BLOCK
        moved = sum(1 for h in self.holes for r in h if lo <= r < hi)
        full = False
        if self.k["small_table"] and self.C > 0:
            if self.extents >= 2:             # the table is full: one copy of the cache, then extents again
                full, self.extents = True, 0
            self.extents += 1
        self.C += BLOCK
        self.W -= BLOCK
        self.triggers += 1
        return dict(fired=True, holes_compressed=moved, full_table=full)

    # ---- ops --------------------------------------------------------------------------------------------------------------------
    def step(self, defer=False, lse=None):
        if lse is None:
            lse = bool(self.rng.integers(3) == 0)
        lse = lse and (self.C > 0 or self.k["head_dim"] == 64)
        self.L += 1
        self.W += 1
        c = self.close(defer)
        self.emit("step", lse=lse, **c)
        self.after_defer(c)

    def split(self, frozen=None):
        if self.any_hole():
            frozen = "p"
        elif frozen is None:
            frozen = ("s", "p", "sp")[self.rng.integers(3)]
        self.L += 1
        self.W += 1
        self.emit("split", frozen=frozen, **self.close())

    def after_defer(self, c, pool=False):
        if c.get("defer"):
            self.emit("run_triggers", pool=pool, **self.fire())

    def mask_kind(self, n_q, per_token=None):
        r = self.rng.integers(4)
        kind = ("none", "row", "causal", "tree")[r] if per_token is None else per_token
        if n_q == 1 and kind == "tree":
            kind = "causal"
        if kind == "none" and self.any_hole():
            kind = "row"
        return kind

    def tree(self, n_q):
        """parents[j] < j of a random draft tree (node 0 is the root) and one root-to-node path."""
        parents = [-1] + [j - 1 if self.rng.integers(3) else int(self.rng.integers(max(0, j - 3), j)) for j in range(1, n_q)]
        node, path = int(self.rng.integers(n_q // 2, n_q)), []
        while node >= 0:
            path.append(node)
            node = parents[node]
        return parents, path[::-1]

    def several(self, op, n_q, mask=None, accept=None, frozen=None, defer=False, pool=False, lse=None):
        """A multi / multi_split op of n_q tokens and the accept that closes it.  accept: None (random), "all", ("rejected", r),
        "unequal"."""
        assert 1 <= n_q <= self.rem(), "a call would step over a trigger point"
        mask = self.mask_kind(n_q, mask)
        parents, path = self.tree(n_q) if mask == "tree" else (None, None)
        L0 = self.L
        # ---- what stays: `keep` (None: accept(rejected=)) and, per sequence, the new rows it accepts
        if accept is None:
            if mask == "tree":
                accept = "unequal" if self.rng.integers(3) == 0 else "path"
            else:
                accept = ("rejected", "prefix", "unequal")[self.rng.integers(3)]
                if accept == "rejected":
                    accept = ("rejected", int(self.rng.integers(0, min(4, n_q))))
        if accept == "unequal" and (n_q < 2 or (mask == "tree" and len(path) < 2)):
            accept = "path" if mask == "tree" else ("rejected", 0)
        assert mask != "tree" or accept in ("path", "unequal"), "a tree is closed along one path"
        keep, rejected = None, 0
        if accept == "all":       # every row stays: rejected=0, or keep= naming them all
            if self.rng.integers(2):
                keep = [list(range(n_q))] * B
            accepted = [set(range(n_q))] * B
        elif isinstance(accept, tuple):
            rejected = accept[1]
            accepted = [set(range(n_q - rejected))] * B
        elif accept == "path":
            keep = [list(path)] * B
            accepted = [set(path)] * B
        elif accept == "prefix":
            keep = [list(range(int(self.rng.integers(max(1, n_q - 3), n_q + 1))))] * B
            accepted = [set(keep[0])] * B
        else:   # unequal: one sequence accepts less than the other and pads with nodes it rejected
            order = list(path) if mask == "tree" else list(range(int(self.rng.integers(max(2, n_q - 2), n_q + 1))))
            short = int(self.rng.integers(1, len(order)))
            loser = int(self.rng.integers(B))
            spare = [j for j in range(n_q) if j not in order[:short]]
            pad = [spare[int(self.rng.integers(len(spare)))] for _ in range(len(order) - short)]
            keep = [order[:short] + pad if b == loser else list(order) for b in range(B)]
            accepted = [set(order[:short]) if b == loser else set(order) for b in range(B)]
            self.unequal_done = True
        poison = [sorted(set(range(n_q)) - a) for a in accepted]
        fields = dict(n_q=n_q, mask=mask, parents=parents, poison=poison)
        self.L += n_q
        self.W += n_q
        due = trigger_due(self.L, self.C, self.W)
        if op == "multi":
            self.emit("multi", lse=bool(self.rng.integers(2)) if lse is None else lse, last_row_is_point=due, **fields)
        else:
            if frozen is None:
                frozen = ("s", "p", "sp")[self.rng.integers(3)]
            self.emit("multi_split", frozen=frozen, last_row_is_point=due, **fields)
        # ---- the accept
        new_holes = [[], []]
        if keep is None:
            self.L -= rejected
            self.W -= rejected
            a = dict(rejected=rejected, keep=None, n_q=n_q)
        else:
            n_keep = len(keep[0])
            for b in range(B):
                for i, j in enumerate(keep[b]):
                    if j not in accepted[b]:      # a pad: the row stays, the sequence rejected it
                        new_holes[b].append(L0 + i)
                        self.holes[b].add(L0 + i)
            self.L -= n_q - n_keep
            self.W -= n_q - n_keep
            a = dict(rejected=0, keep=keep, n_q=n_q)
        c = self.close(defer)
        self.emit("accept", new_holes=new_holes, unequal=accept == "unequal", closes=op, **a, **c)
        self.after_defer(c, pool)

    # ---- a session ----------------------------------------------------------------------------------------------------------------
    def random_op(self):
        room = min(20, self.rem() - 2)        # the filling never touches the trigger point nor the row before it
        kinds = ["step", "multi", "multi", "multi"] + (["split", "multi_split"] if self.split_ok() else [])
        op = kinds[self.rng.integers(len(kinds))]
        if op == "step":
            self.step()
        elif op == "split":
            self.split()
        else:
            self.several(op, int(self.rng.integers(min(4, room), room + 1)))

    def forced(self, period):
        """The ops a period must hold, in a shuffled order behind the ones whose order matters."""
        k, first = self.k, []
        if self.split_ok() and not self.any_hole():
            first += [lambda: self.split("s"), lambda: self.split("sp"), lambda: self.split("s")]
        if not self.unequal_done and (k["split"] is None or self.split_ok()):
            first.append(lambda: self.several("multi", int(self.rng.integers(3, 7)), mask=("causal", "row")[period % 2], accept="unequal"))
        rest = []
        if self.split_ok():
            rest += [lambda: self.split(), lambda: self.split(),
                     lambda: self.several("multi_split", int(self.rng.integers(2, 13))),
                     lambda: self.several("multi_split", int(self.rng.integers(13, 21))),
                     lambda: self.several("multi_split", 1, frozen=("s", "sp")[period % 2], mask="row")]
        big = max(self.per + 1, 17)           # more than one library call (beyond 20 tokens only where 64 // groups is)
        if period == 2:
            rest.append(lambda: self.several("multi", int(self.rng.integers(big, big + 4)), mask="causal"))
        if period == 3:
            rest.append(lambda: self.several("multi", int(self.rng.integers(big, big + 4)), mask="tree"))
        if period == 4:
            rest.append(lambda: self.several("multi", int(self.rng.integers(big, big + 4)), mask=("causal", "tree")[self.rng.integers(2)]))
        self.rng.shuffle(rest)
        return first + rest

    def arrive(self, mode, defer=False, pool=False):
        """From 2 .. 20 rows short of the trigger point to the trigger."""
        rem = self.rem()
        assert 2 <= rem <= 20
        plain = lambda: ("none", "row", "causal")[self.rng.integers(3)]      # (a tree is closed along a path: rows would go)
        if mode == "A":        # a multi whose last row is the trigger point; accept() fires
            self.several("multi", rem, accept="all", defer=defer, pool=pool, mask=plain())
        elif mode == "B1":     # ... its last draft rejected: one row short; a single step fires
            self.several("multi", rem, accept=("rejected", 1), mask=plain())
            assert self.rem() == 1
            self.step(defer=defer)
        elif mode == "B2":     # ... or a one-token decode_multi
            self.several("multi", rem, accept=("rejected", 1), mask=plain())
            self.several("multi", 1, accept="all", defer=defer, pool=pool, mask=plain())
        elif mode == "C":      # a multi_split whose last row is the trigger point
            self.several("multi_split", rem, accept="all", mask=plain())
        else:                  # D: single-token calls
            self.several("multi", rem - 1, accept="all", mask=plain())
            self.split() if self.split_ok() else self.step()

    def run(self):
        k = self.k
        two = k["layers"] == 2
        modes = {1: ("B1", False, False), 2: ("A", two, two), 3: ("A" if two else ("C" if k["split"] else "B2"), False, False),
                 4: ("B1" if two else "D", two, False)}
        for period in range(1, TRIGGERS + 1):
            for f in self.forced(period):
                if self.rem() > 45 + (self.per if self.per > 20 else 0):
                    f()
            while self.rem() > 20:
                self.random_op()
            mode, defer, pool = modes[period]
            self.arrive(mode, defer, pool)
            assert self.triggers == period
        # the tail: calls over the cache the last trigger left
        if self.split_ok():
            self.several("multi_split", int(self.rng.integers(2, 9)), frozen="sp")
        for _ in range(5):
            self.random_op()
        return self.ops


def plan(kind, seed):
    """The ops of session (kind, seed): deterministic."""
    return _Planner(kind, seed).run()
