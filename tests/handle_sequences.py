"""Model-based call sequences over the three handle types (docs/ACCURACY.md, "Handle state: seeded call sequences").

A seeded generator draws a sequence of calls.  The sequence runs on ONE long-lived handle; after every call, what the call
returned is compared bit for bit with what the same call returns on a FRESH TWIN that was brought to the same logical
state by the canonical route: the shortest call list that determines the state.  The claim under test: nothing else a
handle has lived through leaves a trace.

The module is plain Python over numpy: it never imports the library.  `run(subject, factory, seed, steps)` takes the
classes from `factory` -- cugp_amd.gp on the GPU (tests/test_gpu_handle_sequences.py), tests/standin_handles.py on the CPU
(tests/test_handle_sequences_cpu.py) -- which must offer Covsum, SparseGP and BCM with the library's method names.

Three pieces per subject:

  op table   name -> (draw(rng, model, gen) -> keyword arguments, apply(sub, handle, model, **kw) -> [(label, value)]).
             Arguments are small integers (seeds, indices, sizes): the arrays are made from them by the Subject's
             deterministic helpers, so a printed op list is all that is needed to replay a failure by hand.
  model      the logical state, derived from the library's code (the line numbers are in docs/ACCURACY.md), with
             advance(op, result) and route() -> the canonical call list of a twin.
  deck       the multiset of ops one sequence is a shuffle of: every op class is in it, so every seed runs them all.

Where the library documents that two routes to "the same" state give different bits BY DESIGN, the route keeps the
distinction:
  * Covsum / BCM experts: the gradient continued from a valid factor (compute_loglikelihood, then a call that needs the
    inverse) equals the combined evaluation to rounding only (tests/test_gpu_parity.py::
    test_gradient_continues_from_a_valid_factor), so the LEVEL is part of the route;
  * Covsum.append extends a valid inverse in place, chunk by chunk (tests/truth_append.py): the chunks applied since the
    level became full are part of the route;
  * an optimiser leaves the handle at the point of its last probe or stale at its end point, which only its own run can
    tell: the optimiser call itself becomes part of the route, and so does every level call behind it, until the next
    call that makes the handle stale or evaluates it from scratch.

The poison shapes (docs/ACCURACY.md, "When the covariance cannot be factored") run the same decks with steps that take a
handle into the failed state -- a covariance that cannot be factored: NaN results with CUGP_OK -- and out again.  On
them alone NaN agrees with NaN whatever its payload; the shapes, decks, seeds and op lists shipped before are unchanged.
"""
import zlib

import numpy as np

import numerical_failure as nf
from conftest import synth

REFUSED = -1                     # CUGP_ERR_INVALID: the one error code that is an observation ("the call was refused")
TILE = 128


# ------------------------------------------------------------------------------------------------ ops and observations
class Op:
    __slots__ = ("name", "kw")

    def __init__(self, name, **kw):
        self.name, self.kw = name, kw

    def __repr__(self):
        return "%s(%s)" % (self.name, ", ".join("%s=%r" % kv for kv in self.kw.items()))


class Mismatch(AssertionError):
    """A call on the long-lived handle did not return the bits of the same call on the fresh twin."""


def observe(fn):
    """-> ("ok", [(label, value)]) or ("refused", message): only the library's CUGP_ERR_INVALID (a stand-in raises a
    RuntimeError with the same .code) is an observation; every other error is the test's failure."""
    try:
        return ("ok", fn())
    except RuntimeError as e:
        if getattr(e, "code", None) != REFUSED:
            raise
        return ("refused", str(e))


def bits(v):
    """A value as a flat uint64 array: fp64 through a view (NaN payloads and the sign of zero count), None as empty."""
    if v is None:
        return np.zeros(0, dtype=np.uint64)
    a = np.ascontiguousarray(v)
    if a.dtype.kind in "iub":
        return a.astype(np.uint64).ravel()
    return np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)


def first_difference(got, want, nan_equal=False):
    """None when two observations agree bit for bit, else a description of the first output that does not.
    nan_equal (the poison shapes alone): NaN on both sides agrees whatever its sign and payload (nf.same_bits_nan);
    every finite value still agrees in bits."""
    if got[0] != want[0]:
        return "the long-lived handle %s, the twin %s" % (_brief(got), _brief(want))
    if got[0] == "refused":
        return None if got[1] == want[1] else "refusals differ: %r against %r" % (got[1], want[1])
    if [l for l, _ in got[1]] != [l for l, _ in want[1]]:
        return "outputs differ: %r against %r" % ([l for l, _ in got[1]], [l for l, _ in want[1]])
    for (label, a), (_, b) in zip(got[1], want[1]):
        if np.shape(a) != np.shape(b):
            return "output %r: shape %r against %r" % (label, np.shape(a), np.shape(b))
        ba, bb = bits(a), bits(b)
        differ = ba != bb
        if nan_equal and np.asarray(a).dtype.kind == "f" and np.asarray(b).dtype.kind == "f":
            differ &= ~(np.isnan(ba.view(np.float64)) & np.isnan(bb.view(np.float64)))
        bad = np.flatnonzero(differ)
        if bad.size:
            i = int(bad[0])
            fa, fb = ba[i:i + 1].view(np.float64)[0], bb[i:i + 1].view(np.float64)[0]
            return "output %r differs at flat index %d (%d of %d entries differ): %.17g against the twin's %.17g" % (
                label, i, bad.size, ba.size, fa, fb)
    return None


def _brief(obs):
    return "was refused (%s)" % obs[1] if obs[0] == "refused" else "returned %s" % ([l for l, _ in obs[1]],)


def _show(call):
    name, args, kw = call
    parts = ["<%s>" % "x".join(str(s) for s in a.shape) if isinstance(a, np.ndarray) and a.size > 8 else
             repr(a.tolist() if isinstance(a, np.ndarray) else a) for a in args]
    parts += ["%s=%r" % kv for kv in kw.items()]
    return "%s(%s)" % (name, ", ".join(parts))


def call(name, *args, **kw):
    return (name, args, kw)


def replay(h, route):
    """Apply a route to a handle; ("view", k, name) entries go to expert k's view of a BCM."""
    for name, args, kw in route:
        if name == "view":
            getattr(h.expert(args[0]), args[1])()
        else:
            getattr(h, name)(*args, **kw)


# ------------------------------------------------------------------------------------------------ subjects
class Subject:
    """One shape of one handle type: how to create it, the arrays behind the ops' integer arguments, its deck."""

    def __init__(self, name, kind, deck, seeds, steps, **shape):
        self.name, self.kind, self.deck, self.seeds, self.steps = name, kind, deck, tuple(seeds), steps
        self.salt = zlib.crc32(name.encode()) % 1000
        self.poison, self.hp_bad = False, None       # a poison shape: its deck has the *_bad steps; NaN agrees with NaN
        self.__dict__.update(shape)

    # -- arrays from integers
    def rows(self, seed, n, stream=1):
        return synth(n, d=self.d, seed=100000 * stream + 1000 * self.salt + seed, scale=self.scale)

    def points(self, seed, nt):
        """nt test points in the box of the data."""
        Xt = synth(nt, d=self.d, seed=300000 + 1000 * self.salt + seed, scale=self.scale)[0]
        return np.ascontiguousarray(Xt)

    def targets(self, X, seed, m):
        rng = np.random.default_rng(400000 + 1000 * self.salt + seed)
        A = rng.standard_normal((self.d, m)) * (0.5 / np.sqrt(self.d))
        if self.poison:                              # targets stay finite over a poisoned row of X: the repair of X is a repair
            X = np.nan_to_num(X)
        return np.ascontiguousarray(np.sin(X @ A) + 0.1 * rng.standard_normal((X.shape[0], m)))

    def normals(self, seed, ns, nt):
        return np.random.default_rng(500000 + seed).standard_normal((ns, nt))

    def hp_of(self, idx):
        return np.array(self.hps[idx], dtype=np.float64)

    def model(self):
        return MODELS[self.kind](self)

    def ops(self):
        return TABLES[self.kind]


def generate(sub, seed, steps=None):
    """The op list of (subject, seed): the deck shuffled, arguments drawn as the model's dry run goes along.  Needs no
    handle: an optimiser's end point, which only a run can tell, never enters a draw."""
    steps = sub.steps if steps is None else steps
    rng = np.random.default_rng([sub.salt, seed])
    names = list(sub.deck)
    rng.shuffle(names)
    while len(names) < steps:
        names.append(sub.deck[int(rng.integers(len(sub.deck)))])
    model, gen, out = sub.model(), {"rot": int(rng.integers(1 << 16))}, []
    table = sub.ops()
    for name in names[:steps]:
        op = Op(name, **table[name][0](rng, model, gen))
        out.append(op)
        model.advance(op, None)
    return out


def run(sub, factory, seed, steps=None, log=print):
    """Run (subject, seed) on the classes of `factory`; raises Mismatch with everything needed to replay by hand.
    -> the op list."""
    ops = generate(sub, seed, steps)
    table, model = sub.ops(), sub.model()
    live = model.create(factory)
    try:
        replay(live, model.route())
        for i, op in enumerate(ops):
            apply = table[op.name][1]
            got = observe(lambda: apply(sub, live, model, **op.kw))
            route = model.route()
            twin = model.create(factory)
            try:
                replay(twin, route)
                want = observe(lambda: apply(sub, twin, model, **op.kw))
            finally:
                twin.close()
            diff = first_difference(got, want, nan_equal=sub.poison)
            if diff is not None:
                raise Mismatch(
                    "%s seed %d step %d: %r\n  %s\n  ops so far:\n    %s\n  route of the twin (%s):\n    %s" % (
                        sub.name, seed, i, op, diff, "\n    ".join("%2d %r" % (j, o) for j, o in enumerate(ops[:i + 1])),
                        model.describe(), "\n    ".join(_show(c) for c in [model.creation()] + route)))
            model.advance(op, got)
            if log:
                log("SEQ %s %d %d %s %s %s" % (sub.name, seed, i, op.name,
                                               ",".join("%s=%s" % kv for kv in op.kw.items()) or "-",
                                               "ok" if got[0] == "ok" else "ok(refused)"))
    finally:
        live.close()
    return ops


def _res(result, label):
    """An output of an op's observation by label (None in the generator's dry run, or when the call was refused)."""
    if result is None or result[0] != "ok":
        return None
    return dict(result[1]).get(label)


def _stays_put(model, result):
    """An optimiser started on a poisoned handle: its first evaluation is NaN, so is its search direction and every probe
    (minimize.cpp: cg_loop's start, :192-197, and the halving of a NaN step, :210-215), no probe is better than the start
    and the handle ends where it began -- hp (and Z) keep their bits, which the generator's dry run can rely on.  -> True
    then (checked against the run's own end point where there is one); False for a healthy start."""
    if not model.poisoned:
        return False
    for label, held in (("end", model.hp), ("Z", getattr(model, "Z", None))):
        seen = _res(result, label)
        if seen is not None and not nf.same_bits_nan(seen, held):
            raise AssertionError("an optimiser started on a poisoned handle moved %r: %r against %r" % (label, seen, held))
    return True


def _cycle(gen, key, values):
    """The i-th draw of `key` in one sequence walks `values` from an offset the sequence's seed fixed."""
    i = gen.get(key, 0)
    gen[key] = i + 1
    return values[(gen["rot"] + i) % len(values)]


# ================================================================================================ Covsum
LL, LG = call("compute_loglikelihood"), call("loglik_grad")
NT_PRED = (257, 1, 130, 64, 65)                # the scratch shared by predict / predict_latent / predict_grad
NT_JOINT = (65, 1, 130)
TARGET_M = (1, 3, 130, 5)                      # 130: across the 128-column boundary; 5 -> 1: the padded width stays
APPEND_K = (1, 3, 64)


class CovsumModel:
    """capacity, family, (X, y) over the current rows, hp, targets -- and how the handle got its factor:
    base_n rows and base_hp were current when the handle was last stale; `tail` are the level calls since."""

    def __init__(self, sub):
        self.sub = sub
        self.X, self.y = sub.rows(0, sub.n0)
        self.hp, self.hp_idx = sub.hp_of(0), 0
        self.hp_poison = False                       # the hyper-parameters are the subject's hp_bad (hp_idx -1)
        self.Y = None
        self._reset()

    n = property(lambda self: len(self.y))
    # K cannot be factored: every evaluation is a failed one (NaN results, CUGP_OK) until a repair
    poisoned = property(lambda self: self.hp_poison or bool(np.isnan(self.X).any()))
    cap = property(lambda self: (max(self.sub.n0, self.sub.npad_min) + TILE - 1) // TILE * TILE)

    def _reset(self):
        self.base_n, self.base_hp, self.tail = self.n, self.hp, []

    @property
    def level(self):
        t = self.tail
        if any(c[0].startswith("cg_solve") for c in t):
            return "opt"
        if not t:
            return "stale"
        if t[0] == LG:
            return "full"
        return "factor" if len(t) == 1 else "full_cont"

    def describe(self):
        return "level %s, n %d (base %d), targets %s" % (self.level, self.n, self.base_n,
                                                         "none" if self.Y is None else self.Y.shape[1])

    def creation(self):
        s = self.sub
        return call("Covsum", self.base_n, s.d, npad_min=s.npad_min, ard=s.ard, kernel=s.kernel)

    def create(self, factory):
        _, args, kw = self.creation()
        return factory.Covsum(*args, **kw)

    def route(self):
        r = [call("set_data", self.X[:self.base_n], self.y[:self.base_n]), call("set_loghyperparam", self.base_hp)]
        for c in self.tail:
            r.append(call("append", self.X[c[1][0]:c[1][1]], self.y[c[1][0]:c[1][1]]) if c[0] == "append" else c)
        if self.Y is not None:
            r.append(call("set_targets", self.Y))
        return r

    # -- the transitions (cugp_capi.cpp: cugp_loglik, cugp_loglik_grad, enqueue_eval, set_theta; dense_features.cpp: cugp_append)
    def _loglik(self):
        if self.level == "stale":
            self.tail = [LL]
        elif self.level == "opt":
            self.tail.append(LL)

    def _inverse(self):
        lv = self.level
        if lv == "stale":
            self.tail = [LG]
        elif lv in ("factor", "opt"):
            self.tail.append(LG)

    def append_refused(self, k):
        return "targets" if self.Y is not None else "capacity" if self.n + k > self.cap else None

    def advance(self, op, result):
        name, kw, s = op.name, op.kw, self.sub
        if name in ("set_data", "set_data_bad"):
            self.X, self.y = s.rows(kw["seed"], self.n)
            if name == "set_data_bad":
                self.X = nf.poison_row(self.X, kw["row"])
            self._reset()
        elif name == "set_hp":
            if self.hp_idx != kw["idx"]:
                self.hp, self.hp_idx, self.hp_poison = s.hp_of(kw["idx"]), kw["idx"], False
                self._reset()
        elif name == "set_hp_bad":
            if self.hp_idx != -1:
                self.hp, self.hp_idx, self.hp_poison = np.array(s.hp_bad, dtype=np.float64), -1, True
                self._reset()
        elif name in ("compute_K_train", "compute_squared_dist", "detour"):
            self._reset()
        elif name == "compute_loglikelihood":
            self._loglik()
        elif name in NEEDS_INVERSE or (name in NEEDS_TARGETS and self.Y is not None):
            self._inverse()
        elif name == "enqueue_fetch":
            self._reset()
            self.tail = [LG if kw["grad"] else LL]
        elif name == "set_targets":
            self.Y = s.targets(self.X, kw["seed"], kw["cols"])
        elif name == "append":
            if self.append_refused(kw["k"]) is None:
                lo = self.n
                Xa, ya = s.rows(kw["seed"], kw["k"], stream=2)
                self.X, self.y = np.concatenate([self.X, Xa]), np.concatenate([self.y, ya])
                # (a poisoned handle that holds its -- NaN -- inverse borders it, finds LL not finite and keeps nothing:
                #  the discard_eval at the end of cugp_append, dense_features.cpp; behind an optimiser the twin replays the append)
                if self.level == "opt" or (self.level in ("full", "full_cont") and not self.poisoned):
                    self.tail.append(("append", (lo, self.n)))
                else:
                    self._reset()
        elif name in ("cg_solve", "cg_solve_loo"):
            self.tail.append(call(name, budget=kw["budget"]))
            if not _stays_put(self, result):
                self.hp, self.hp_idx = _res(result, "end"), None


NEEDS_INVERSE = ("loglik_grad", "compute_gradient_loghyperparam", "predict", "predict_latent", "predict_grad",
                 "compute_test_joint", "sample_posterior", "loo", "loo_predict")
NEEDS_TARGETS = ("loglik_grad_targets", "predict_targets", "get_alpha_targets")
READS = ("get_cholesky", "get_K_inverse", "get_alpha", "last_quad_logdet")


def _other_hp(rng, m):
    choices = [i for i in range(len(m.sub.hps)) if i != m.hp_idx]
    return int(choices[int(rng.integers(len(choices)))])


def _none(rng, m, gen):
    return {}


def _cv_append_draw(rng, m, gen):
    k = int(APPEND_K[int(rng.integers(len(APPEND_K)))])
    if m.Y is None and m.n + k > m.sub.nmax:                      # the model has grown as far as it goes: ask for more
        k = m.cap - m.n + 1                                       # rows than the handle has room for -- a refusal
    return {"k": k, "seed": int(rng.integers(1000))}


def _cv_detour(s, h, m, away, grad):
    back = h.get_loghyperparam()
    h.set_loghyperparam(s.hp_of(away))
    out = _ll_g(h.loglik_grad()) if grad else [("ll", h.compute_loglikelihood())]
    h.set_loghyperparam(back)
    return out


def _ll_g(r):
    return [("ll", r[0]), ("g", r[1])]


def _cv_enqueue_fetch(s, h, m, grad):
    h.enqueue(want_grad=grad)
    ll, g = h.fetch()
    return [("ll", ll), ("g", g)] if grad else [("ll", ll)]      # (without the gradient, g is the last one's: history)


def _cv_cg(name):
    def apply(s, h, m, budget):
        tr = getattr(h, name)(budget=budget)
        return [("trace", tr), ("end", h.get_loghyperparam())]
    return apply


def _named(labels, fn):
    def apply(s, h, m, **kw):
        r = fn(s, h, m, **kw)
        return list(zip(labels, r if isinstance(r, tuple) else (r,)))
    return apply


def _nothing(fn):
    def apply(s, h, m, **kw):
        fn(s, h, m, **kw)
        return []
    return apply


COVSUM_OPS = {
    "set_data": (lambda rng, m, gen: {"seed": int(rng.integers(1, 1000))},
                 _nothing(lambda s, h, m, seed: h.set_data(*s.rows(seed, m.n)))),
    "set_hp": (lambda rng, m, gen: {"idx": _other_hp(rng, m)},
               _nothing(lambda s, h, m, idx: h.set_loghyperparam(s.hp_of(idx)))),
    "set_hp_same": (_none, _nothing(lambda s, h, m: h.set_loghyperparam(m.hp.copy()))),
    "compute_loglikelihood": (_none, _named(("ll",), lambda s, h, m: h.compute_loglikelihood())),
    "loglik_grad": (_none, _named(("ll", "g"), lambda s, h, m: h.loglik_grad())),
    "compute_gradient_loghyperparam": (_none, _named(("g",), lambda s, h, m: h.compute_gradient_loghyperparam())),
    "enqueue_fetch": (lambda rng, m, gen: {"grad": bool(rng.integers(2))}, _cv_enqueue_fetch),
    "predict": (lambda rng, m, gen: {"nt": _cycle(gen, "pred", NT_PRED), "pts": int(rng.integers(100))},
                _named(("mean", "var"),
                       lambda s, h, m, nt, pts: h.compute_test_means_and_variances(None, None, s.points(pts, nt)))),
    "predict_latent": (lambda rng, m, gen: {"nt": _cycle(gen, "pred", NT_PRED), "pts": int(rng.integers(100))},
                       _named(("mean", "var"), lambda s, h, m, nt, pts: h.predict_latent(s.points(pts, nt)))),
    "predict_grad": (lambda rng, m, gen: {"nt": _cycle(gen, "pred", NT_PRED), "pts": int(rng.integers(100)),
                                          "noise": bool(rng.integers(2))},
                     _named(("mean", "var", "dmean", "dvar"),
                            lambda s, h, m, nt, pts, noise: h.predict_grad(s.points(pts, nt), with_noise=noise))),
    "compute_test_joint": (lambda rng, m, gen: {"nt": _cycle(gen, "joint", NT_JOINT), "pts": int(rng.integers(100)),
                                                "noise": bool(rng.integers(2))},
                           _named(("mean", "cov"), lambda s, h, m, nt, pts, noise: h.compute_test_joint(
                               None, None, s.points(pts, nt), with_noise=noise))),
    "sample_posterior": (lambda rng, m, gen: {"nt": _cycle(gen, "joint", NT_JOINT), "pts": int(rng.integers(100)),
                                              "noise": bool(rng.integers(2))},
                         _named(("draws",), lambda s, h, m, nt, pts, noise: h.sample_posterior(
                             None, None, s.points(pts, nt), 2, with_noise=noise, jitter=0.0,
                             normals=s.normals(pts, 2, nt)))),
    "loo": (lambda rng, m, gen: {"grad": bool(rng.integers(2))},
            _named(("lpl", "g"), lambda s, h, m, grad: h.loo(want_grad=grad))),
    "loo_predict": (_none, _named(("mean", "var", "logp"), lambda s, h, m: h.loo_predict())),
    "get_cholesky": (_none, _named(("L",), lambda s, h, m: h.get_cholesky())),
    "get_K_inverse": (_none, _named(("Kinv",), lambda s, h, m: h.get_K_inverse())),
    "get_alpha": (_none, _named(("alpha",), lambda s, h, m: h.get_alpha())),
    "last_quad_logdet": (_none, _named(("quad", "logdet"), lambda s, h, m: h.last_quad_logdet())),
    "set_targets": (lambda rng, m, gen: {"cols": _cycle(gen, "tg", TARGET_M), "seed": int(rng.integers(1000))},
                    _nothing(lambda s, h, m, cols, seed: h.set_targets(s.targets(m.X, seed, cols)))),
    "loglik_grad_targets": (_none, _named(("ll", "g", "each"), lambda s, h, m: h.loglik_grad_targets())),
    "predict_targets": (lambda rng, m, gen: {"nt": int(NT_PRED[int(rng.integers(len(NT_PRED)))]),
                                             "pts": int(rng.integers(100))},
                        _named(("mean", "var"), lambda s, h, m, nt, pts: h.predict_targets(s.points(pts, nt)))),
    "get_alpha_targets": (_none, _named(("A",), lambda s, h, m: h.get_alpha_targets())),
    "compute_K_train": (_none, _named(("K",), lambda s, h, m: h.compute_K_train())),
    "compute_k_test": (lambda rng, m, gen: {"nt": int(NT_PRED[int(rng.integers(len(NT_PRED)))]),
                                            "pts": int(rng.integers(100))},
                       _named(("Ks",), lambda s, h, m, nt, pts: h.compute_k_test(s.points(pts, nt)))),
    "compute_squared_dist": (lambda rng, m, gen: {"c": float(rng.integers(1, 5)) / 2},
                             _named(("S",), lambda s, h, m, c: h.compute_squared_dist(c))),
    "append": (_cv_append_draw,
               _nothing(lambda s, h, m, k, seed: h.append(*s.rows(seed, k, stream=2)))),
    "detour": (lambda rng, m, gen: {"away": _other_hp(rng, m), "grad": bool(rng.integers(2))}, _cv_detour),
    "cg_solve": (lambda rng, m, gen: {"budget": 3}, _cv_cg("cg_solve")),
    "cg_solve_loo": (lambda rng, m, gen: {"budget": 3}, _cv_cg("cg_solve_loo")),
}

_COVSUM_ONCE = [n for n in COVSUM_OPS if n not in ("append", "compute_squared_dist")]
DECK_COVSUM_FIXED_N = _COVSUM_ONCE + ["set_hp", "compute_loglikelihood", "predict", "predict", "loglik_grad",
                                     "set_targets", "set_targets", "set_targets"]
DECK_COVSUM = DECK_COVSUM_FIXED_N + ["compute_squared_dist"] + ["append"] * 4


# -- the poison steps (docs/ACCURACY.md, "When the covariance cannot be factored"): into the failed state and, by the
# existing set_hp / set_data, out of it.  Added behind the decks above, which list the table: those stay as they were.
def _bad_rows(rng, m, gen):
    return {"seed": int(rng.integers(1, 1000)), "row": int(rng.integers(m.n))}


def _set_hp_bad(setter):
    return (_none, _nothing(lambda s, h, m: getattr(h, setter)(np.array(s.hp_bad, dtype=np.float64))))


POISON_OPS = ("set_hp_bad", "set_data_bad", "set_expert_data_bad", "set_inducing_bad")
COVSUM_OPS.update({
    "set_hp_bad": _set_hp_bad("set_loghyperparam"),
    "set_data_bad": (_bad_rows, _nothing(lambda s, h, m, seed, row: h.set_data(
        nf.poison_row(s.rows(seed, m.n)[0], row), s.rows(seed, m.n)[1]))),
})
# the existing deck, the poison steps and as many repairs again
DECK_COVSUM_POISON = DECK_COVSUM + ["set_hp_bad"] * 3 + ["set_data_bad"] * 3 + ["set_hp"] * 3 + ["set_data"] * 3


# ================================================================================================ SparseGP
SP_NT = (257, 1, 65)
SP_NT_JOINT = (65, 1)
SP_P = (1, 3, 17)
SP_OWN = ("bound", "bound_grad", "bound_grad_z", "predict", "predict_joint", "predict_grad", "sample_posterior",
          "cg_solve", "cg_solve_z")
SP_TG = ("bound_targets", "bound_grad_targets", "bound_grad_z_targets", "predict_targets", "cg_solve_targets")


class SparseModel:
    """(X, y), Z, hp, targets.  Every evaluation of a side starts from the covariance of Z (sp_eval, sparse.cpp: a side
    is valid or evaluated afresh; evaluating one marks the other stale), so the twin is: fresh, data, Z, hp, targets."""

    def __init__(self, sub):
        self.sub = sub
        self.X, self.y = sub.rows(0, sub.n)
        self.Z = self.X[sub.zrows(0)].copy()
        self.hp, self.hp_idx = sub.hp_of(0), 0
        self.Y = None
        self.last_side = None
        self.hp_poison = False

    # Kuu (a NaN row of Z, hp_bad) or B (a NaN row of X) cannot be factored.  A failed evaluation of a side is an evaluation:
    # it leaves the side valid over a NaN row and the other side stale (sp_eval, sparse.cpp: the early return for Kuu,
    # the end of the function for B), and predictions of a side that is not `pd` are NaN (sp_predict) -- nothing the twin's route lacks.
    # (Z is None in the generator's dry run behind an optimiser over Z that started healthy: it ended at finite values)
    poisoned = property(lambda self: self.hp_poison or bool(np.isnan(self.X).any()) or
                        (self.Z is not None and bool(np.isnan(self.Z).any())))

    def describe(self):
        return "targets %s%s" % ("none" if self.Y is None else self.Y.shape[1], ", poisoned" if self.poisoned else "")

    def creation(self):
        s = self.sub
        return call("SparseGP", s.n, s.m, s.d, kernel=s.kernel, ard=s.ard, chunk_rows=s.chunk_rows)

    def create(self, factory):
        _, args, kw = self.creation()
        return factory.SparseGP(*args, **kw)

    def route(self):
        r = [call("set_data", self.X, self.y), call("set_inducing", self.Z), call("set_loghyperparam", self.hp)]
        if self.Y is not None:
            r.append(call("set_targets", self.Y))
        return r

    def advance(self, op, result):
        name, kw, s = op.name, op.kw, self.sub
        if name in ("set_data", "set_data_bad"):
            self.X, self.y = s.rows(kw["seed"], s.n)
            if name == "set_data_bad":
                self.X = nf.poison_row(self.X, kw["row"])
        elif name in ("set_inducing", "set_inducing_bad"):
            self.Z = self.X[s.zrows(kw["seed"])] + kw["shift"]
            if name == "set_inducing_bad":
                self.Z = nf.poison_row(self.Z, kw["row"])
        elif name == "set_hp":
            self.hp, self.hp_idx, self.hp_poison = s.hp_of(kw["idx"]), kw["idx"], False
        elif name == "set_hp_bad":
            self.hp, self.hp_idx, self.hp_poison = np.array(s.hp_bad, dtype=np.float64), -1, True
        elif name == "set_targets":
            self.Y = s.targets(self.X, kw["seed"], kw["p"])
        elif name.startswith("cg_solve") and (name != "cg_solve_targets" or self.Y is not None):
            if not _stays_put(self, result):
                self.hp, self.hp_idx = _res(result, "end"), None
                if name == "cg_solve_z" or kw.get("inducing"):
                    self.Z = _res(result, "Z")


def _sp_cg(method, inducing):
    def apply(s, h, m, budget, **kw):
        tr = getattr(h, method)(budget=budget, inducing=kw.get("inducing", inducing))
        return [("trace", tr), ("end", h.get_loghyperparam()), ("Z", h.get_inducing())]
    return apply


def _sp_pts(cycle):
    return lambda rng, m, gen: {"nt": _cycle(gen, "pred", cycle), "pts": int(rng.integers(100)),
                                "noise": bool(rng.integers(2))}


SPARSE_OPS = {
    "set_data": (lambda rng, m, gen: {"seed": int(rng.integers(1, 1000))},
                 _nothing(lambda s, h, m, seed: h.set_data(*s.rows(seed, s.n)))),
    "set_inducing": (lambda rng, m, gen: {"seed": int(rng.integers(1000)), "shift": float(rng.integers(0, 3)) / 8},
                     _nothing(lambda s, h, m, seed, shift: h.set_inducing(m.X[s.zrows(seed)] + shift))),
    "set_hp": (lambda rng, m, gen: {"idx": _other_hp(rng, m)},
               _nothing(lambda s, h, m, idx: h.set_loghyperparam(s.hp_of(idx)))),
    "set_hp_same": (_none, _nothing(lambda s, h, m: h.set_loghyperparam(m.hp.copy()))),
    "bound": (_none, _named(("F",), lambda s, h, m: h.bound())),
    "bound_grad": (_none, _named(("F", "g"), lambda s, h, m: h.bound_grad())),
    "bound_grad_z": (_none, _named(("F", "g", "gZ"), lambda s, h, m: h.bound_grad_z())),
    "predict": (_sp_pts(SP_NT), _named(("mean", "var"),
                                       lambda s, h, m, nt, pts, noise: h.predict(s.points(pts, nt), with_noise=noise))),
    "predict_joint": (lambda rng, m, gen: {"nt": _cycle(gen, "joint", SP_NT_JOINT), "pts": int(rng.integers(100)),
                                           "noise": bool(rng.integers(2))},
                      _named(("mean", "cov"), lambda s, h, m, nt, pts, noise: h.predict_joint(s.points(pts, nt),
                                                                                             with_noise=noise))),
    "predict_grad": (_sp_pts(SP_NT), _named(("mean", "var", "dmean", "dvar"), lambda s, h, m, nt, pts, noise:
                                            h.predict_grad(s.points(pts, nt), with_noise=noise))),
    "sample_posterior": (lambda rng, m, gen: {"nt": _cycle(gen, "joint", SP_NT_JOINT), "pts": int(rng.integers(100)),
                                              "noise": bool(rng.integers(2))},
                         _named(("draws",), lambda s, h, m, nt, pts, noise: h.sample_posterior(
                             s.points(pts, nt), 2, with_noise=noise, jitter=0.0 if noise else 1e-8,
                             normals=s.normals(pts, 2, nt)))),
    "set_targets": (lambda rng, m, gen: {"p": _cycle(gen, "tg", SP_P), "seed": int(rng.integers(1000))},
                    _nothing(lambda s, h, m, p, seed: h.set_targets(s.targets(m.X, seed, p)))),
    "bound_targets": (_none, _named(("F", "each"), lambda s, h, m: h.bound_targets())),
    "bound_grad_targets": (_none, _named(("F", "g", "each"), lambda s, h, m: h.bound_grad_targets())),
    "bound_grad_z_targets": (_none, _named(("F", "g", "gZ", "each"), lambda s, h, m: h.bound_grad_z_targets())),
    "predict_targets": (_sp_pts(SP_NT), _named(("mean", "var"), lambda s, h, m, nt, pts, noise:
                                               h.predict_targets(s.points(pts, nt), with_noise=noise))),
    "cg_solve_targets": (lambda rng, m, gen: {"budget": 3, "inducing": bool(rng.integers(2))},
                         _sp_cg("cg_solve_targets", False)),
    "get_inducing": (_none, _named(("Z",), lambda s, h, m: h.get_inducing())),
    "cg_solve": (lambda rng, m, gen: {"budget": 3}, _sp_cg("cg_solve", False)),
    "cg_solve_z": (lambda rng, m, gen: {"budget": 3}, _sp_cg("cg_solve", True)),
}

DECK_SPARSE = list(SPARSE_OPS) + ["set_data", "set_inducing", "set_hp", "bound", "bound_grad", "bound_grad_z", "predict",
                                  "predict", "predict", "predict_joint", "predict_grad", "sample_posterior",
                                  "set_targets", "set_targets", "bound_targets", "bound_grad_targets",
                                  "bound_grad_z_targets", "predict_targets", "predict_targets", "get_inducing"]

SPARSE_OPS.update({
    "set_hp_bad": _set_hp_bad("set_loghyperparam"),
    "set_data_bad": (lambda rng, m, gen: {"seed": int(rng.integers(1, 1000)), "row": int(rng.integers(m.sub.n))},
                     _nothing(lambda s, h, m, seed, row: h.set_data(nf.poison_row(s.rows(seed, s.n)[0], row),
                                                                    s.rows(seed, s.n)[1]))),
    "set_inducing_bad": (lambda rng, m, gen: {"seed": int(rng.integers(1000)), "shift": float(rng.integers(0, 3)) / 8,
                                              "row": int(rng.integers(m.sub.m))},
                         _nothing(lambda s, h, m, seed, shift, row: h.set_inducing(
                             nf.poison_row(m.X[s.zrows(seed)] + shift, row)))),
})
DECK_SPARSE_POISON = (DECK_SPARSE + ["set_hp_bad"] * 2 + ["set_data_bad"] * 2 + ["set_inducing_bad"] * 2 +
                      ["set_hp"] * 2 + ["set_data"] * 2 + ["set_inducing"] * 2)


# ================================================================================================ BCM
BCM_NT = (130, 1, 65, 64)
COMBINE = ("poe", "gpoe", "bcm", "rbcm")
VIEW_LL, VIEW_LG = "compute_loglikelihood", "loglik_grad"
EVAL = call("loglik_grad")


class BCMModel:
    """Per expert: the data seed and a Covsum level; the shared hp.  base_seeds and base_hp were current when every expert
    was last stale or the whole model was last evaluated; `tail` are the calls since that moved an expert's level.
    A BCM evaluation (cugp_group_enqueue / cugp_loglik_grad_enqueue, bcm.cpp: bcm_enqueue_all) drops every expert's
    factor and evaluates all of them from their data, whatever came before; a prediction evaluates the whole model when one
    expert lacks its inverse (bcm_refresh) and otherwise reads the experts as they are -- an expert view's own continued
    gradient included."""

    def __init__(self, sub):
        self.sub = sub
        self.K = len(sub.rows_per_expert)
        self.seeds = [0] * self.K                    # per expert: its data seed, or (seed, row) with that row of X NaN
        self.hp, self.hp_idx = sub.hp_of(0), 0
        self.hp_poison = False
        self._reset()

    # one expert that cannot be factored: the sums of an evaluation are NaN, that expert's level moves as any other's
    # (read_result_row, cugp_capi.cpp, sets factor_valid and inverse_valid whatever the row holds)
    poisoned = property(lambda self: self.hp_poison or any(isinstance(sd, tuple) for sd in self.seeds))

    def _reset(self, tail=()):
        self.base_seeds, self.base_hp, self.tail = list(self.seeds), self.hp, list(tail)
        self.levels = ["full" if tail else "stale"] * self.K

    def data(self, k, seed):
        if isinstance(seed, tuple):
            X, y = self.data(k, seed[0])
            return nf.poison_row(X, seed[1]), y
        return self.sub.rows(1000 * (k + 1) + seed, self.sub.rows_per_expert[k])

    def describe(self):
        return "levels %s" % ",".join(self.levels)

    def creation(self):
        s = self.sub
        return call("BCM", list(s.rows_per_expert), s.d, kernel=s.kernel, ard=s.ard)

    def create(self, factory):
        _, args, kw = self.creation()
        return factory.BCM(*args, **kw)

    def route(self):
        r = [call("set_expert_data", k, *self.data(k, self.base_seeds[k])) for k in range(self.K)]
        r.append(call("set_BCM_log_hyperparam", self.base_hp))
        for c in self.tail:
            r.append(call("set_expert_data", c[1][0], *self.data(*c[1])) if c[0] == "data" else
                     call("compute_BCM_test_means_and_var", self.sub.points(0, 1)) if c[0] == "refresh" else c)
        return r

    opt = property(lambda self: any(c[0] == "cg_solve" for c in self.tail))

    def _view(self, k, need_inverse):
        lv = self.levels[k]
        calls = {("stale", False): "factor", ("stale", True): "full", ("factor", True): "full_cont"}
        if lv == "opt":
            self.tail.append(call("view", k, VIEW_LG if need_inverse else VIEW_LL))
        elif (lv, need_inverse) in calls:
            self.levels[k] = calls[(lv, need_inverse)]
            self.tail.append(call("view", k, VIEW_LG if need_inverse else VIEW_LL))

    def advance(self, op, result):
        name, kw = op.name, op.kw
        if name in ("set_expert_data", "set_expert_data_bad"):
            k = kw["k"]
            seed = kw["seed"] if name == "set_expert_data" else (kw["seed"], kw["row"])
            self.seeds[k] = seed
            if not self.tail:
                self.base_seeds[k] = seed
            else:
                if not self.opt:                                   # (behind an optimiser its path needs every call, in order)
                    self.tail = [c for c in self.tail if not (c[0] in ("view", "data") and c[1][0] == k)]
                self.tail.append(("data", (k, seed)))
            self.levels[k] = "stale"
        elif name == "set_hp":
            if self.hp_idx != kw["idx"]:
                self.hp, self.hp_idx, self.hp_poison = self.sub.hp_of(kw["idx"]), kw["idx"], False
                self._reset()
        elif name == "set_hp_bad":
            if self.hp_idx != -1:
                self.hp, self.hp_idx, self.hp_poison = np.array(self.sub.hp_bad, dtype=np.float64), -1, True
                self._reset()
        elif name in ("loglik_grad", "loglik_grad_rows"):
            self._reset([EVAL])
        elif name in ("bcm_predict", "predict", "predict_grad"):
            if any(lv in ("stale", "factor") for lv in self.levels):
                self._reset([EVAL])
            elif "opt" in self.levels:
                self.tail.append(("refresh", ()))
        elif name == "view_loglik":
            self._view(kw["k"], False)
        elif name in ("view_loglik_grad", "view_predict"):
            self._view(kw["k"], True)
        elif name == "cg_solve":
            self.tail.append(call("cg_solve", budget=kw["budget"]))
            self.levels = ["opt"] * self.K
            if not _stays_put(self, result):
                self.hp, self.hp_idx = _res(result, "end"), None


def _bcm_k(rng, m, gen):
    return {"k": int(rng.integers(m.K))}


def _bcm_pts(rng, m, gen):
    return {"nt": _cycle(gen, "pred", BCM_NT), "pts": int(rng.integers(100))}


def _bcm_cg(s, h, m, budget):
    tr = h.cg_solve(budget=budget)
    return [("trace", tr), ("end", h.get_loghyperparam())]


BCM_OPS = {
    "set_expert_data": (lambda rng, m, gen: {"k": int(rng.integers(m.K)), "seed": int(rng.integers(1, 1000))},
                        _nothing(lambda s, h, m, k, seed: h.set_expert_data(k, *m.data(k, seed)))),
    "set_hp": (lambda rng, m, gen: {"idx": _other_hp(rng, m)},
               _nothing(lambda s, h, m, idx: h.set_BCM_log_hyperparam(s.hp_of(idx)))),
    "set_hp_same": (_none, _nothing(lambda s, h, m: h.set_BCM_log_hyperparam(m.hp.copy()))),
    "loglik_grad": (_none, _named(("ll", "g", "each"), lambda s, h, m: h.loglik_grad())),
    "loglik_grad_rows": (_none, _named(("rows",), lambda s, h, m: h.loglik_grad_rows())),
    "bcm_predict": (_bcm_pts, _named(("mean", "var"),
                                     lambda s, h, m, nt, pts: h.compute_BCM_test_means_and_var(s.points(pts, nt)))),
    "predict": (lambda rng, m, gen: dict(_bcm_pts(rng, m, gen), combine=_cycle(gen, "rule", COMBINE),
                                         noise=bool(rng.integers(2))),
                _named(("mean", "var"), lambda s, h, m, nt, pts, combine, noise:
                       h.predict(s.points(pts, nt), combine=combine, with_noise=noise))),
    "predict_grad": (lambda rng, m, gen: dict(_bcm_pts(rng, m, gen), combine=_cycle(gen, "grule", (None,) + COMBINE),
                                              noise=bool(rng.integers(2))),
                     _named(("mean", "var", "dmean", "dvar"), lambda s, h, m, nt, pts, combine, noise:
                            h.predict_grad(s.points(pts, nt), combine=combine, with_noise=noise))),
    "view_loglik": (_bcm_k, _named(("ll",), lambda s, h, m, k: h.expert(k).compute_loglikelihood())),
    "view_loglik_grad": (_bcm_k, _named(("ll", "g"), lambda s, h, m, k: h.expert(k).loglik_grad())),
    "view_predict": (lambda rng, m, gen: dict(_bcm_pts(rng, m, gen), k=int(rng.integers(m.K))),
                     _named(("mean", "var"), lambda s, h, m, nt, pts, k:
                            h.expert(k).compute_test_means_and_variances(None, None, s.points(pts, nt)))),
    "cg_solve": (lambda rng, m, gen: {"budget": 3}, _bcm_cg),
}

DECK_BCM = (["set_expert_data"] * 5 + ["set_hp"] * 2 + ["set_hp_same"] * 2 + ["loglik_grad"] * 5 + ["loglik_grad_rows"] * 3 +
            ["bcm_predict"] * 3 + ["predict"] * 4 + ["predict_grad"] * 4 + ["view_loglik"] * 4 + ["view_loglik_grad"] * 3 +
            ["view_predict"] * 3 + ["cg_solve"] * 2)

BCM_OPS.update({
    "set_hp_bad": _set_hp_bad("set_BCM_log_hyperparam"),
    "set_expert_data_bad": (lambda rng, m, gen: (lambda k: {"k": k, "seed": int(rng.integers(1, 1000)), "row": int(
        rng.integers(m.sub.rows_per_expert[k]))})(int(rng.integers(m.K))),
                            _nothing(lambda s, h, m, k, seed, row: h.set_expert_data(k, *m.data(k, (seed, row))))),
})
DECK_BCM_POISON = DECK_BCM + ["set_hp_bad"] * 3 + ["set_expert_data_bad"] * 3 + ["set_hp"] * 2 + ["set_expert_data"] * 3

MODELS = {"covsum": CovsumModel, "sparse": SparseModel, "bcm": BCMModel}
TABLES = {"covsum": COVSUM_OPS, "sparse": SPARSE_OPS, "bcm": BCM_OPS}


# ================================================================================================ the shipped subjects
def _near(hp):
    """hp moved by less than 1e-9 in its first entry: another point to the library, the same to a tolerant comparison."""
    out = list(hp)
    out[0] = out[0] + 5e-10
    return out


_HP_SE = [0.9, 0.2, -1.0]
_HPS_SE = [_HP_SE, _near(_HP_SE), [0.7, 0.1, -0.8], [1.1, 0.3, -1.2]]
_HP_ARD17 = np.linspace(0.7, 1.9, 17).tolist() + [0.3, -0.8]
_HP_ARD3 = [0.9, 0.3, 1.6, 0.2, -1.0]


def _shifted(hp, by):
    return [h + by for h in hp[:-2]] + list(hp[-2:])


def _zrows(n, m):
    return lambda seed: np.sort(np.random.default_rng(600000 + seed).choice(n, m, replace=False))


# a length scale of exp(-800) = 0: K = k(X, X) has NaN on its diagonal (0 / 0) and zeros beside it -- no pivot is healthy
_HP_BAD = [-800.0, 0.2, -1.0]
# (a greedy search over the seeds 1 .. 399 for poison_coverage's conditions, from the generator alone)
_SEEDS_POISON = {"covsum": (16, 33, 173, 122, 36, 317), "sparse": (92, 25, 68, 211, 321), "bcm": (191, 391, 124)}

SUBJECTS = {s.name: s for s in (
    # (a) three tiles of capacity, the captured graph, an append across the 256-row tile boundary
    Subject("covsum_se_n193", "covsum", DECK_COVSUM, seeds=(5, 6, 65), steps=40, d=3, n0=193, nmax=257, npad_min=384,
            ard=False, kernel="se", scale=4.0, hps=_HPS_SE),
    # (b) ARD, two feature chunks
    Subject("covsum_ard_n300_d17", "covsum", DECK_COVSUM_FIXED_N, seeds=(1,), steps=16, d=17, n0=300, nmax=300,
            npad_min=0, ard=True, kernel="se", scale=1.8,
            hps=[_HP_ARD17, _near(_HP_ARD17), _shifted(_HP_ARD17, -0.1), _shifted(_HP_ARD17, 0.1)]),
    # (c) the multi-stream evaluation
    Subject("covsum_se_n1300_d6", "covsum", DECK_COVSUM_FIXED_N + ["compute_squared_dist"], seeds=(1,), steps=16, d=6,
            n0=1300, nmax=1300, npad_min=0, ard=False, kernel="se", scale=2.5, hps=_HPS_SE),
    # three chunks, the last ragged; mpad padding
    Subject("sparse_se_n300_m65", "sparse", DECK_SPARSE, seeds=(1, 2, 3), steps=40, d=2, n=300, m=65, chunk_rows=128,
            ard=False, kernel="se", scale=4.0, hps=[[0.5, 0.5, 0.5], [0.4, 0.45, 0.4], [0.6, 0.55, 0.3]],
            zrows=_zrows(300, 65)),
    Subject("sparse_matern32_ard_n257_m64", "sparse", DECK_SPARSE, seeds=(1, 2, 43), steps=40, d=3, n=257, m=64,
            chunk_rows=128, ard=False, kernel="matern32_ard", scale=4.0,
            hps=[_HP_ARD3, _shifted(_HP_ARD3, -0.1), _shifted(_HP_ARD3, 0.1)], zrows=_zrows(257, 64)),
    # one group with ragged tiles
    Subject("bcm_se_64_64_66", "bcm", DECK_BCM, seeds=(1, 2, 27), steps=40, d=3, rows_per_expert=(64, 64, 66), ard=False,
            kernel="se", scale=4.0, hps=_HPS_SE),
    # very unequal experts: no group, every expert on its own stream
    Subject("bcm_ard_100_400", "bcm", DECK_BCM, seeds=(1,), steps=16, d=3, rows_per_expert=(100, 400), ard=True,
            kernel="se", scale=4.0, hps=[_HP_ARD3, _near(_HP_ARD3), _shifted(_HP_ARD3, -0.1), _shifted(_HP_ARD3, 0.1)]),
    # the poison shapes: the shapes of (a), the first sparse and the first BCM shape above, their decks with the steps
    # into the failed state and as many repairs again; seeds chosen for poison_coverage's conditions
    Subject("covsum_se_n193_poison", "covsum", DECK_COVSUM_POISON, seeds=_SEEDS_POISON["covsum"],
            steps=len(DECK_COVSUM_POISON), d=3, n0=193, nmax=257, npad_min=384, ard=False, kernel="se", scale=4.0,
            hps=_HPS_SE, poison=True, hp_bad=_HP_BAD),
    Subject("sparse_se_poison", "sparse", DECK_SPARSE_POISON, seeds=_SEEDS_POISON["sparse"],
            steps=len(DECK_SPARSE_POISON), d=2, n=300, m=65, chunk_rows=128, ard=False, kernel="se", scale=4.0,
            hps=[[0.5, 0.5, 0.5], [0.4, 0.45, 0.4], [0.6, 0.55, 0.3]], zrows=_zrows(300, 65), poison=True,
            hp_bad=[-800.0, 0.5, 0.5]),
    Subject("bcm_se_poison", "bcm", DECK_BCM_POISON, seeds=_SEEDS_POISON["bcm"], steps=len(DECK_BCM_POISON), d=3,
            rows_per_expert=(64, 64, 66), ard=False, kernel="se", scale=4.0, hps=_HPS_SE, poison=True, hp_bad=_HP_BAD),
)}

CASES = [(s.name, seed) for s in SUBJECTS.values() for seed in s.seeds]


# ================================================================================================ coverage, from the generator alone
def walk(sub, seed, steps=None):
    """[(op, model level before the op, refusal the model expects or None)] of the generator's dry run."""
    out, model = [], sub.model()
    for op in generate(sub, seed, steps):
        level = getattr(model, "level", None)
        refusal = model.append_refused(op.kw["k"]) if (sub.kind, op.name) == ("covsum", "append") else None
        out.append((op, level, refusal))
        model.advance(op, None)
    return out


def coverage(kind):
    """The coverage conditions of one handle type over its shipped seeds -> {condition: bool}."""
    subs = [s for s in SUBJECTS.values() if s.kind == kind and not s.poison]      # (the poison shapes: poison_coverage)
    walks = [(s, seed, walk(s, seed)) for s in subs for seed in s.seeds]
    counts = {}
    for _, _, w in walks:
        for op, _, _ in w:
            counts[op.name] = counts.get(op.name, 0) + 1
    cond = {"every op class at least twice": all(counts.get(n, 0) >= 2 for n in TABLES[kind] if n not in POISON_OPS)}

    def in_order(seq, tests):
        """some consecutive entries of seq pass tests[0], tests[1], ... in that order"""
        return any(all(t(x) for t, x in zip(tests, seq[i:i + len(tests)]))
                   for i in range(len(seq) - len(tests) + 1))

    if kind == "covsum":
        levels = {lv for _, _, w in walks for op, lv, _ in w if op.name in READS}
        cond["a reading op at each of the four levels"] = {"stale", "factor", "full", "full_cont"} <= levels
        scratch = ("predict", "predict_latent", "predict_grad")
        cond["a prediction at 1 point follows one at 257"] = any(in_order(
            [x for x in w if x[0].name in scratch], [lambda x: x[0].kw["nt"] == 257, lambda x: x[0].kw["nt"] == 1])
            for _, _, w in walks)
        cond["targets go 3 -> 130 -> 5"] = any(in_order(
            [x for x in w if x[0].name == "set_targets"], [lambda x, c=c: x[0].kw["cols"] == c for c in (3, 130, 5)])
            for _, _, w in walks)
        apps = [(lv, ref) for _, _, w in walks for op, lv, ref in w if op.name == "append"]
        cond["an append with a valid inverse"] = any(ref is None and lv in ("full", "full_cont") for lv, ref in apps)
        cond["an append without a valid inverse"] = any(ref is None and lv in ("stale", "factor") for lv, ref in apps)
        cond["an append refused for targets"] = any(ref == "targets" for _, ref in apps)
        cond["an append refused for capacity"] = any(ref == "capacity" for _, ref in apps)
        cond["an append across the 256-row tile boundary"] = any(
            ref is None and before < 256 <= before + op.kw["k"] for _, _, w in walks
            for (op, _, ref), before in zip(w, _rows_before(w, subs[0].n0)) if op.name == "append")
    if kind == "sparse":
        def alternations(w):
            sides = ["own" if op.name in SP_OWN else "tg" for op, _, _ in _with_targets(w) if op.name in SP_OWN + SP_TG]
            return sum(a != b for a, b in zip(sides, sides[1:]))
        cond["own-side and target-side calls alternate at least three times"] = any(alternations(w) >= 3
                                                                                    for _, _, w in walks)
        cond["predictions at 257 points, then at 1"] = any(in_order(
            [x for x in w if x[0].name in ("predict", "predict_grad")],
            [lambda x: x[0].kw["nt"] == 257, lambda x: x[0].kw["nt"] == 1]) for _, _, w in walks)
    if kind == "bcm":
        group = ("loglik_grad", "loglik_grad_rows")
        views = ("view_loglik", "view_loglik_grad", "view_predict")
        cond["an expert-view evaluation between two group evaluations"] = any(in_order(
            [x for x in w if x[0].name in group + views],
            [lambda x: x[0].name in group, lambda x: x[0].name in views, lambda x: x[0].name in group])
            for _, _, w in walks)
    opt = ("cg_solve", "cg_solve_loo", "cg_solve_z", "cg_solve_targets")
    cond["an optimiser with at least five further ops behind it"] = any(
        op.name in opt and len(w) - 1 - i >= 5 for _, _, w in walks for i, (op, _, _) in enumerate(w))
    return cond


def _rows_before(w, n0):
    n, out = n0, []
    for op, _, ref in w:
        out.append(n)
        if op.name == "append" and ref is None:
            n += op.kw["k"]
    return out


def _with_targets(w):
    """the part of a sparse walk from the first set_targets on (before it the target side's calls are refusals)"""
    for i, (op, _, _) in enumerate(w):
        if op.name == "set_targets":
            return w[i:]
    return []


# ================================================================================================ coverage of the poison shapes
# the op classes that evaluate the model when it is stale (the target side's: once targets are set)
EVALUATING = {
    "covsum": NEEDS_INVERSE + ("compute_loglikelihood", "enqueue_fetch", "detour", "cg_solve", "cg_solve_loo"),
    "sparse": SP_OWN,
    "bcm": ("loglik_grad", "loglik_grad_rows", "bcm_predict", "predict", "predict_grad", "view_loglik", "view_loglik_grad",
            "view_predict", "cg_solve"),
}
EVALUATING_WITH_TARGETS = {"covsum": NEEDS_TARGETS, "sparse": SP_TG, "bcm": ()}


def poison_walk(sub, seed, steps=None):
    """[(op, poisoned before the op, poisoned after it, targets set before it)] of the generator's dry run."""
    out, model = [], sub.model()
    for op in generate(sub, seed, steps):
        before, targets = model.poisoned, getattr(model, "Y", None) is not None
        model.advance(op, None)
        out.append((op, before, model.poisoned, targets))
    return out


def poison_sets(sub, seed):
    """(op classes seen while the handle was poisoned, op classes seen as the first evaluating call after a repair) of
    one sequence.  A repair is a step that takes a poisoned handle to a healthy one; the first evaluating call after it
    counts only if nothing poisoned the handle again in between."""
    evaluating = EVALUATING[sub.kind]
    while_poisoned, after_repair, waiting = set(), set(), False
    for op, before, after, targets in poison_walk(sub, seed):
        if before:
            while_poisoned.add(op.name)
        if waiting and not before and (op.name in evaluating or
                                       (targets and op.name in EVALUATING_WITH_TARGETS[sub.kind])):
            after_repair.add(op.name)
            waiting = False
        if before and not after:
            waiting = True
        elif after:
            waiting = False
    return while_poisoned, after_repair


def poison_coverage(name):
    """The coverage conditions of one poison shape over its shipped seeds -> {condition: bool}."""
    sub = SUBJECTS[name]
    seen, first = set(), set()
    for seed in sub.seeds:
        a, b = poison_sets(sub, seed)
        seen |= a
        first |= b
    classes = set(sub.deck)
    evaluating = set(EVALUATING[sub.kind] + EVALUATING_WITH_TARGETS[sub.kind]) & classes
    return {"every op class while the handle is poisoned": classes <= seen,
            "every evaluating op class as the first evaluating call after a repair": evaluating <= first}
