"""The call-sequence harness (tests/handle_sequences.py) has teeth -- checked without a GPU, on the fp64 stand-ins of
tests/standin_handles.py:

  1. the shipped seeds find no mismatch on the clean stand-ins;
  2. each of the ten staleness mutations is caught by a shipped seed (the seed and the step are printed: pytest -s), and
     each of the two mutations of the failed state by a shipped seed of a poison shape;
  3. the coverage conditions hold for the shipped seeds -- asserted from the generator alone;
  4. the sequences shipped before the poison shapes are the sequences they were.

docs/ACCURACY.md, "Handle state: seeded call sequences", keeps the tables.
"""
import zlib

import numpy as np
import pytest

import handle_sequences as hs
import standin_handles as sh

KINDS = ("covsum", "sparse", "bcm")
# mutation -> the handle type whose sequences must catch it
MUTATION_KIND = dict.fromkeys(sh.MUTATIONS, "covsum")
MUTATION_KIND.update(sparse_sides_independent="sparse", set_inducing_keeps_row_z="sparse",
                     expert_data_keeps_sum="bcm", view_taken_for_group="bcm", sparse_kuu_failure_keeps_row="sparse")
# the mutations of the failed state: only a sequence with poison steps can see them
POISON_MUTATIONS = ("failed_eval_keeps_gradient", "sparse_kuu_failure_keeps_row")
POISON_SHAPES = [name for name, sub in hs.SUBJECTS.items() if sub.poison]


@pytest.fixture(autouse=True)
def clean_standins():
    sh.ACTIVE.clear()
    yield
    sh.ACTIVE.clear()


@pytest.mark.parametrize("name,seed", hs.CASES, ids=["%s-%d" % c for c in hs.CASES])
def test_clean_standins_give_no_mismatch(name, seed):
    sub = hs.SUBJECTS[name]
    ops = hs.run(sub, sh, seed, log=None)
    assert len(ops) == sub.steps


@pytest.mark.parametrize("mutation", sh.MUTATIONS)
def test_mutation_is_caught(mutation):
    """One invalidation switched off in the stand-ins: some shipped seed of the handle type must report a mismatch."""
    sh.ACTIVE.add(mutation)
    caught = []
    for name, seed in hs.CASES:
        sub = hs.SUBJECTS[name]
        if sub.kind != MUTATION_KIND[mutation] or sub.poison != (mutation in POISON_MUTATIONS):
            continue
        try:
            hs.run(sub, sh, seed, log=None)
        except hs.Mismatch as e:
            caught.append(str(e).split("\n")[0])
    print("MUTATION %-34s caught at: %s" % (mutation, "; ".join(caught) or "nowhere"))
    assert caught, "no shipped seed notices the mutation %r" % mutation


@pytest.mark.parametrize("kind", KINDS)
def test_coverage_conditions(kind):
    cond = hs.coverage(kind)
    for name, holds in cond.items():
        print("COVERAGE %-7s %-62s %s" % (kind, name, "holds" if holds else "MISSING"))
    assert all(cond.values()), [name for name, holds in cond.items() if not holds]


@pytest.mark.parametrize("name", POISON_SHAPES)
def test_poison_coverage_conditions(name):
    """Over the shipped seeds of a poison shape every op class of its deck runs at least once while the handle is poisoned,
    and every op class that evaluates at least once as the first evaluating call after a repair."""
    cond = hs.poison_coverage(name)
    for what, holds in cond.items():
        print("COVERAGE %-22s %-70s %s" % (name, what, "holds" if holds else "MISSING"))
    assert all(cond.values()), [what for what, holds in cond.items() if not holds]
    sub = hs.SUBJECTS[name]
    assert len(sub.seeds) >= 3 and set(sub.deck) & set(hs.POISON_OPS)


# crc32 of the printed op lists of the sequences shipped before the poison shapes were added
SHIPPED = {("covsum_se_n193", 5): 1339509551, ("covsum_se_n193", 6): 3326302704, ("covsum_se_n193", 65): 485253555,
           ("covsum_ard_n300_d17", 1): 3723631829, ("covsum_se_n1300_d6", 1): 1172591388,
           ("sparse_se_n300_m65", 1): 1234167520, ("sparse_se_n300_m65", 2): 1312503903,
           ("sparse_se_n300_m65", 3): 2481173137, ("sparse_matern32_ard_n257_m64", 1): 2817142880,
           ("sparse_matern32_ard_n257_m64", 2): 3341951677, ("sparse_matern32_ard_n257_m64", 43): 433631626,
           ("bcm_se_64_64_66", 1): 1582028731, ("bcm_se_64_64_66", 2): 72659259, ("bcm_se_64_64_66", 27): 2937741551,
           ("bcm_ard_100_400", 1): 3069169235}


def test_shipped_sequences_are_unchanged():
    assert [c for c in hs.CASES if not hs.SUBJECTS[c[0]].poison] == list(SHIPPED)
    for (name, seed), crc in SHIPPED.items():
        ops = hs.generate(hs.SUBJECTS[name], seed)
        assert zlib.crc32("\n".join(repr(o) for o in ops).encode()) == crc, (name, seed)
        assert not set(o.name for o in ops) & set(hs.POISON_OPS)


def test_every_op_of_a_table_is_in_a_deck():
    for kind in KINDS:
        decks = set()
        for sub in hs.SUBJECTS.values():
            if sub.kind == kind:
                decks |= set(sub.deck)
        assert decks == set(hs.TABLES[kind]), kind


def test_generation_is_deterministic_and_needs_no_handle():
    for name, seed in hs.CASES:
        a, b = hs.generate(hs.SUBJECTS[name], seed), hs.generate(hs.SUBJECTS[name], seed)
        assert [repr(o) for o in a] == [repr(o) for o in b]


def test_a_mismatch_report_can_be_replayed_by_hand():
    """The report of a mismatch names the seed, the step, the ops so far and the twin's route; replaying the printed op
    list on a handle and the printed route on a fresh one shows the same difference."""
    sh.ACTIVE.add("hp_keeps_targets")
    sub, report = None, None
    for name, seed in hs.CASES:
        if hs.SUBJECTS[name].kind != "covsum":
            continue
        try:
            hs.run(hs.SUBJECTS[name], sh, seed, log=None)
        except hs.Mismatch as e:
            sub, report = hs.SUBJECTS[name], str(e)
            break
    assert report is not None
    head = report.split("\n")[0]
    seed, step = int(head.split(" seed ")[1].split()[0]), int(head.split(" step ")[1].split(":")[0])
    assert "ops so far:" in report and "route of the twin" in report and "differs at flat index" in report
    ops = hs.generate(sub, seed)[:step + 1]
    assert [repr(o) for o in ops] == [line.split(None, 1)[1] for line in
                                      report.split("ops so far:\n")[1].split("\n  route")[0].strip().split("\n    ")]
    model, table = sub.model(), sub.ops()
    live = model.create(sh)
    hs.replay(live, model.route())
    for op in ops[:-1]:
        model.advance(op, hs.observe(lambda: table[op.name][1](sub, live, model, **op.kw)))
    got = hs.observe(lambda: table[ops[-1].name][1](sub, live, model, **ops[-1].kw))
    twin = model.create(sh)
    hs.replay(twin, model.route())
    want = hs.observe(lambda: table[ops[-1].name][1](sub, twin, model, **ops[-1].kw))
    assert hs.first_difference(got, want) is not None


def test_bit_comparison_counts_nan_payloads_and_signed_zeros():
    a = np.array([np.nan, 0.0, 1.0])
    b = a.copy()
    assert hs.first_difference(("ok", [("x", a)]), ("ok", [("x", b)])) is None
    b.view(np.uint64)[0] ^= 1                                        # another NaN payload
    assert "index 0" in hs.first_difference(("ok", [("x", a)]), ("ok", [("x", b)]))
    assert "index 1" in hs.first_difference(("ok", [("x", a)]), ("ok", [("x", np.array([np.nan, -0.0, 1.0]))]))
    assert hs.first_difference(("refused", "a"), ("ok", [])) is not None
