"""The inputs of tests/test_gpu_proposal_regime.py do what their names say -- measured on the float64 oracle, on the CPU -- and the float64
criterion reference reproduces torch's BCELoss backward on the planted scores."""
import numpy as np
import pytest
import torch

from oracle import echr_ref_cpu as O
from tests import proposal_regime_ref as P


def _one(p, y, w1=0.25):
    """d loss / d p of one element (T = K = 1, mask 1) through oracle.tap_criterion in float64."""
    s = torch.tensor([[p]], dtype=torch.float64, requires_grad=True)
    O.tap_criterion(s, torch.ones(1, 1, dtype=torch.float64), torch.tensor([[float(y)]], dtype=torch.float64),
                    torch.tensor([w1], dtype=torch.float64)).backward()
    return float(s.grad)


# (p, y, torch BCELoss' d loss / d p at w1 = 0.25: (p - y) / max(p (1 - p), 1e-12) * w, w = 0.75 under label 1 and 0.25 under label 0)
TORCH_TABLE = [(0.0, 0, 0.0), (0.0, 1, -7.5e11), (1.0, 0, 2.5e11), (1.0, 1, 0.0), (1e-13, 0, 0.025), (1e-13, 1, -7.5e11), (1e-20, 1, -7.5e11)]


@pytest.mark.parametrize('p,y,want', TORCH_TABLE)
def test_float64_criterion_reference_is_torchs_backward_with_its_floor(p, y, want):
    got = _one(p, y)          # (torch holds the floor as the float32 constant 1e-12f = 1e-12 (1 - 4.0e-9), in float64 too)
    assert abs(got - want) <= 1e-8 * abs(want), (p, y, got, want)


def test_float64_criterion_reference_on_every_planted_element():
    """The reference of the GPU test, element by element, against the closed form in float64 numpy: (p - y) / max(p (1 - p), 1e-12) w m K / n."""
    inp = P.bce_inputs((4,), 16)          # n = 64 >= 48: every planted element is there
    assert len(inp['planted']) == len(P.PLANT) and len(set(inp['planted'].tolist())) == len(P.PLANT)
    losses, g = P.bce_reference(inp)
    sc, mk, lb = (inp[k].astype(np.float64) for k in ('scores', 'masks', 'labels'))
    w1 = inp['w1'][0].astype(np.float64)[None, :]
    p, y = sc * mk, lb * mk
    w = y * (1 - w1) + (1 - y) * w1
    want = P.G_LOSS * w * (p - y) / np.maximum(p * (1 - p), 1e-12) * mk / 4
    assert P.elem_ratio(g, want) <= 1e-8          # (4.0e-9: torch's floor is the float32 constant 1e-12f)
    assert np.isfinite(g).all() and np.abs(g).max() > 1e9 and np.abs(g[g != 0]).min() < 1e-2          # the span a max-norm would hide
    # the forward: the denormal's log is not clamped, the smallest denormal's is
    assert np.log(float(np.float32(1e-40))) > -100 > np.log(float(np.float32(1e-45)))
    term = -np.where(y > 0, np.maximum(np.log(np.maximum(p, 1e-320)), -100), np.maximum(np.log(np.maximum(1 - p, 1e-320)), -100)) * w
    assert abs(losses[0] - term.sum() / 4) <= 1e-12 * losses[0]


def test_float32_numpy_form_of_torchs_backward_stays_inside_the_gate():
    """The formula the kernel evaluates, in float32 numpy, against float64 on every planted value: within 1.0e-7 relative -- two decades inside
    the 1e-5 element gate."""
    worst = 0.0
    for s, y, _ in P.PLANT:
        p32, y32 = np.float32(s), np.float32(y)
        d32 = (p32 - y32) / np.maximum(p32 * (np.float32(1) - p32), np.float32(1e-12))
        d64 = (float(s) - y) / max(float(s) * (1.0 - float(s)), 1e-12)
        worst = max(worst, abs(float(d32) - d64) / max(abs(d64), 1e-300))
    assert worst <= 1.0e-7, worst


def test_gates_sat_saturates_the_gates():
    r = P.probe('gates_sat', batch=True)
    g = r['gates'][0]
    share = float(np.mean((g < 0.01) | (g > 0.99)))
    assert share >= 0.20, share          # (0.33 measured: pre-activation standard deviation 4.6)
    assert int((r['scores32'] == 1.0).sum()) >= 1          # a few scores round to exactly 1.0 in float32


def test_drift_walks_the_cell_state_far_past_one():
    r = P.probe('drift', batch=False)
    assert all(float(np.abs(c).max()) >= 10.0 for c in r['c']), [float(np.abs(c).max()) for c in r['c']]          # (14 and 70 measured)
    # tanh(c) saturates there: 1 - tanh^2 is 0 in float32
    assert np.float32(1) - np.tanh(np.float32(10.0)) ** 2 == 0


def test_bce_chain_stays_below_the_point_where_float32_bce_breaks():
    r = P.probe('bce_chain', batch=True)
    z = float(np.abs(r['z']).max())
    assert 10.0 <= z < 14.0, z          # (12.5 measured)
    assert not (r['scores32'] == 0.0).any() and not (r['scores32'] == 1.0).any()


def test_every_gate_stays_inside_the_contract():
    from tests import test_gpu_proposal_regime as G
    assert set(G.E_REF) == set(P.VARIANTS)
    for name in P.VARIANTS:
        assert max(4 * e for e in G.E_REF[name]) <= G.CONTRACT, name
        assert max(G.gates(name)) <= G.CONTRACT


@pytest.mark.parametrize('train', [False, True])
def test_e_ref_of_the_small_variant_is_what_the_table_says(train):
    """The one variant cheap enough to re-measure in the suite (tools/parity_report.py --sst reprints all of them): the float32 oracle against the
    float64 oracle stays in the decade of the table's entry (its last bits depend on the host's summation order) and inside the contract."""
    from tests import test_gpu_proposal_regime as G
    for batch in (False, True):
        e = P.e_ref('small_h', train, batch)
        assert all(a <= 2 * b for a, b in zip(e[:4], G.E_REF['small_h'])) and 4 * max(e[:4]) <= G.CONTRACT, (batch, e)


def test_selection_grid_repeats_every_class_and_splits_one_from_its_predecessor():
    g = P.saturated_grid(40, 32)
    c = P.class_counts(g)
    assert min(c) >= 8 and sum(c) == sum(min(n + 1, 32) for n in range(40))
    assert P.ONE.view(np.uint32) == 0x3F800000 and P.PRED.view(np.uint32) == 0x3F7FFFFF and P.PRED2.view(np.uint32) == 0x3F7FFFFE
    d = P.I_DENORMAL
    assert 0 < float(P.CLASSES[d]) < 2.0 ** -126 == float(P.CLASSES[d - 1]) and float(P.CLASSES[d + 1]) == 0.0          # a denormal below the smallest normal
    assert all(a > b for a, b in zip(P.CLASSES[:-1], P.CLASSES[1:]))
