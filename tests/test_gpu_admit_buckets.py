"""Length buckets inside a pool admission (csrc/ttx_admit.h: admit_chunks): the rows of one admission are encoded in consecutive
sub-chunks, each at the width of its own longest row, instead of all at the width of the admission's longest row.  A row's encoder
output, cross K/V and drafts do not depend on the padding of the launch that computed them, so TTX_ADMIT_ROWS (the padded rows at
which a sub-chunk closes; 0: one chunk, as before) may change the counters of padded work and nothing else.  Every check is exact
equality: outputs, traces and finish steps between a budget that splits every admission and 0, the tokens against the goldens,
and src_tokens_padded against the rule restated here wherever the call is a single admission (rows <= capacity, one pool).

The rule: an admission of n rows whose n x width is below the budget stays one chunk.  Otherwise rows join the open sub-chunk
until its rows x (longest row so far, at least 2) reaches the budget, which closes it; what is left at the end becomes a sub-chunk
of its own, or joins the one before it when its rows x width is below half the budget."""
import ctypes as C

import pytest
import torch

from util_admit import padded_rows
from util_draft_select import h4_gen, h4_state
from util_models import BOS, EOS, PAD, fixture_tokens, load_npz, tiny_state, upto_eos

pytestmark = pytest.mark.gpu
MAX_LEN, N_DRAFTS, D_LEN = 150, 3, 10


@pytest.fixture(scope="module")
def tta():
    import translation_transformer_amd as t
    assert t.lib().ttx_device_count() >= 1, "no gfx950 device: the HIP path must not be skipped silently"
    return t


@pytest.fixture(scope="module", params=["tiny", "h4"])
def model(request, tta):
    if request.param == "tiny":
        st, cfg = tiny_state()
        gold = load_npz("gen_spec_greedy.npz")["b1_n3_d10_tokens"]
    else:
        st, cfg = h4_state()
        gold = h4_gen()["b1_n3_d10_tokens"]
    m = tta.NativeTransformer(st, cfg["num_heads"], 0, device=0)
    yield m, gold
    m.close()


def lengths_of(src):
    return ((src != PAD) * torch.arange(1, src.shape[1] + 1)).amax(dim=1).tolist()


def pool_call(m, src_rows, capacity, c_token):
    """ttx_greedy_speculative_generate_pool on ONE session over the rows in the order given."""
    from translation_transformer_amd import _native as NA
    src = src_rows.to(m.device, torch.int64).contiguous()
    R, width = src.shape
    out = torch.empty((R, MAX_LEN), dtype=torch.int64, device=src.device)
    traj = torch.empty((R, MAX_LEN + 1), dtype=torch.int16, device=src.device)
    fin = torch.empty((R,), dtype=torch.int32, device=src.device)
    sess = (C.c_void_p * 1)(m.session_pool(1)[0].value)
    p = NA.GenParams(MAX_LEN, D_LEN, N_DRAFTS, PAD, BOS, EOS, c_token, 0)
    st = NA.GenStats()
    rc = m._lib.ttx_greedy_speculative_generate_pool(sess, 1, src.data_ptr(), R, width, (C.c_int32 * R)(*lengths_of(src_rows)), capacity,
                                                     C.byref(p), out.data_ptr(), traj.data_ptr(), fin.data_ptr(), C.byref(st), m._stream())
    torch.cuda.synchronize()
    return out.cpu(), traj.cpu(), fin.cpu(), st, rc


COUNTERS = ["model_calls", "accepted_tokens", "produced_tokens", "verified_positions", "kv_prefix_positions"]


def both_budgets(monkeypatch, m, src_rows, capacity, c_token, budget, rcs=(0,)):
    """The same call with sub-chunks closed at `budget` padded rows and with one chunk per admission: identical results."""
    monkeypatch.setenv("TTX_ADMIT_ROWS", str(budget))
    got = pool_call(m, src_rows, capacity, c_token)
    monkeypatch.setenv("TTX_ADMIT_ROWS", "0")
    one = pool_call(m, src_rows, capacity, c_token)
    assert got[4] == one[4] and got[4] in rcs, (got[4], one[4], m._lib.ttx_last_error())
    for name, a, b in zip(("out", "traj", "fin_step"), got, one):
        assert torch.equal(a, b), f"{name} differs between TTX_ADMIT_ROWS={budget} and 0"
    for k in COUNTERS:                                                  # which rows ran which steps did not change either
        assert getattr(got[3], k) == getattr(one[3], k), k
    return got, one


def by_length(rows, idx):
    """Longest first, as generate_many(reorder=True) hands a list to the pool."""
    order = sorted(range(len(idx)), key=lambda i: -lengths_of(rows[i:i + 1])[0])
    return rows[order], [idx[i] for i in order]


def short_rows(fsrc, n, length):
    """n sources that are the first `length` tokens of fixture rows: not in the goldens, compared between the budgets only."""
    r = torch.zeros((n, fsrc.shape[1]), dtype=fsrc.dtype)
    r[:, :length] = fsrc[torch.arange(n) % fsrc.shape[0], :length]
    return r


def test_mixed_lengths_many_admissions(monkeypatch, model):
    """200 rows of ten lengths between 28 and 127 through 64 slots: the first admission takes 64 rows, the later ones at least 16 while
    the list lasts, and a budget of 140 padded rows splits 16 rows into three sub-chunks or more."""
    m, gold = model
    fsrc, _, c, _ = fixture_tokens()
    idx = (torch.randperm(200, generator=torch.Generator().manual_seed(3)) % 10).tolist()
    rows, idx = by_length(fsrc[idx], idx)
    lens = lengths_of(rows)
    assert min(16 * l for l in lens) >= 3 * 140
    got, one = both_budgets(monkeypatch, m, rows, 64, c, 140)
    out = got[0].numpy()
    for j, r in enumerate(idx):                                         # the golden holds every fixture row decoded alone
        if r >= 0:
            assert upto_eos(out[j]) == upto_eos(gold[r, 0]), (j, r)
    assert sum(lens) <= got[3].src_tokens_padded < one[3].src_tokens_padded
    assert one[3].src_tokens_padded >= padded_rows(lens[:64], 0)[0]


def single_admission(monkeypatch, model, rows, idx, budget, n_chunks, rcs=(0,)):
    """rows <= capacity: one pool, one admission, so src_tokens_padded is the rule's sum over this list."""
    m, gold = model
    _, _, c, _ = fixture_tokens()
    lens = lengths_of(rows)
    want, n = padded_rows(lens, budget)
    assert n == n_chunks, f"the case was built for {n_chunks} sub-chunks, the rule makes {n}"
    got, one = both_budgets(monkeypatch, m, rows, 64, c, budget, rcs)
    assert got[3].src_tokens_padded == want
    assert one[3].src_tokens_padded == len(lens) * max(2, max(lens))
    out = got[0].numpy()
    for j, r in enumerate(idx):
        if r >= 0:
            assert upto_eos(out[j]) == upto_eos(gold[r, 0]), (j, r)


def test_admission_of_a_single_row(monkeypatch, model):
    fsrc = fixture_tokens()[0]
    single_admission(monkeypatch, model, fsrc[6:7], [6], 1, 1)           # 28 tokens against a budget of 1: still one chunk of one row


def test_rows_of_one_length(monkeypatch, model):
    fsrc = fixture_tokens()[0]
    rows = fsrc[[4] * 40]                                               # 40 x 41 tokens: 10 rows reach 400, four full sub-chunks
    single_admission(monkeypatch, model, rows, [4] * 40, 400, 4)


def test_remainder_that_merges(monkeypatch, model):
    """Budget 500: four rows of 127 reach 508, six rows of 91 reach 546.  Four rows of 28 behind them (112 < 250) join the rows of 91
    at their width; nine rows of 28 (252 >= 250) are a sub-chunk of their own."""
    fsrc = fixture_tokens()[0]
    for tail, n_chunks in ((4, 2), (9, 3)):
        idx = [5] * 4 + [1] * 6 + [6] * tail
        single_admission(monkeypatch, model, fsrc[idx], idx, 500, n_chunks)
    assert padded_rows([127] * 4 + [91] * 6 + [28] * 4, 500)[0] == 4 * 127 + 10 * 91


def test_width_of_two(monkeypatch, model):
    """Twelve sources of two tokens behind three long ones, budget 20: every long row is a sub-chunk, ten short rows reach 20 and the
    last two (4 < 10) join them.  That sub-chunk runs at width 2, the smallest the encoder is launched at.  A source of two tokens is
    nothing the models were trained on: they may write a PAD inside such a row, which the pool reports (TTX_ERR_ROW_REPLAY) after it has
    decoded every row, so the comparison between the budgets and the long rows' goldens hold either way."""
    from translation_transformer_amd import _native as NA
    fsrc = fixture_tokens()[0]
    rows = torch.cat([fsrc[[2] * 3], short_rows(fsrc, 12, 2)])
    single_admission(monkeypatch, model, rows, [2] * 3 + [-1] * 12, 20, 4, rcs=(0, NA.TTX_ERR_ROW_REPLAY))
    lens = lengths_of(rows)
    assert padded_rows(lens, 20)[0] == 3 * 76 + 12 * 2
