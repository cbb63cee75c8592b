"""CPU checks of the stochastic beam pool's restatement (tests/util_sbs_pool_checks.py): on an enumerable toy model it returns, for
every capacity from 1 to the number of sources and for shuffled admission orders, exactly the rows, logp and gumbel of the per-source
restatement (tests/util_sbs_checks.py: search), and its checkers flag every planted defect."""
import numpy as np
import pytest

import util_sbs_pool_checks as P

V, PAD, EOS, BOS = 5, 0, 1, 2
K, MAX_LEN, SEED, T = 3, 8, 20190611, 1.0
N_SRC = 7
KEYS = [5, 1 << 40, 7, -3, 0, (1 << 33) + 1, 42]


def toy_model(src: int):
    """Source ``src``'s conditional logits, a fixed function of the prefix; EOS grows likelier with the length and by the source, so
    that sources end at different levels and some reach max_len."""
    def model(rows):
        out = np.empty((len(rows), V), np.float32)
        for i, r in enumerate(rows):
            h = hash((src,) + tuple(int(t) for t in r)) % (2 ** 32)
            x = np.random.default_rng(h).uniform(-1.0, 1.0, V).astype(np.float32)
            x[PAD] = -np.inf
            x[EOS] += np.float32(1.2 * (len(r) - 1) - 2.5 * (src % 4))
            out[i] = x
        return out
    return model


@pytest.fixture(scope="module")
def toy():
    models = [toy_model(i) for i in range(N_SRC)]
    ref = P.reference(models, KEYS, K, MAX_LEN, SEED, T, PAD, BOS, EOS)
    steps = ref[3]
    ended = ((ref[0][:, :, 1:] == EOS) | (ref[0][:, :, 1:] == PAD)).any(-1).all(-1)
    assert len(set(steps[ended].tolist())) >= 3 and (~ended).any(), \
        f"the toy does not stagger retirement: steps {steps.tolist()}, all rows ended {ended.tolist()}"
    return models, ref


def run(models, C, order=None, defect=None, **hooks):
    return P.Pool(models, KEYS, C, K, MAX_LEN, SEED, T, PAD, BOS, EOS, defect=defect).run(order, **hooks)


@pytest.mark.parametrize("C", range(1, N_SRC + 1))
def test_every_capacity_returns_the_per_source_rows(toy, C):
    models, ref = toy
    problems = []
    pool = run(models, C, on_admit=lambda p, first, slots: problems.extend(P.check_admission(p, first, slots)),
               on_iteration=lambda p: problems.extend(P.check_iteration(p)))
    assert not problems, problems
    assert not P.check_outputs(pool, ref)
    assert pool.host["error"] == 0 and pool.host["n_live"] == 0
    assert pool.iteration >= int(ref[3].max()) and (C < N_SRC or pool.iteration == int(ref[3].max()))


@pytest.mark.parametrize("C", [2, 3, 5])
def test_shuffled_admission_orders(toy, C):
    models, ref = toy
    rng = np.random.default_rng(C)
    for _ in range(4):
        order = rng.permutation(N_SRC).tolist()
        assert not P.check_outputs(run(models, C, order), ref), order


def test_running_rows_is_the_sum_over_the_sources(toy):
    """Both loops decode unfinished candidates only, and a retired source has none: the pool's count is the per-source sum."""
    import util_sbs_checks as S
    models, _ = toy
    total = 0
    for m, k in zip(models, KEYS):
        levels = S.search(m, k, SEED, T, K, MAX_LEN, PAD, BOS, EOS)[4]
        total += 1 + sum(int((~lv.finished).sum()) for lv in levels[:-1])
    per_source = [1 + sum(int((~lv.finished).sum()) for lv in S.search(m, k, SEED, T, K, MAX_LEN, PAD, BOS, EOS)[4][:-1])
                  for m, k in zip(models, KEYS)]
    for C in (1, 3, N_SRC):
        pool = run(models, C)
        assert pool.running_rows == total
        assert pool.src_running.tolist() == per_source          # what retirement hands out per source


@pytest.mark.parametrize("defect", P.DEFECTS)
def test_checkers_flag_a_planted_defect(toy, defect):
    models, ref = toy
    problems = []
    pool = run(models, 3, defect=defect, on_admit=lambda p, first, slots: problems.extend(P.check_admission(p, first, slots)),
               on_iteration=lambda p: problems.extend(P.check_iteration(p)))
    problems += P.check_outputs(pool, ref)
    assert problems, f"{defect}: nothing flagged"
