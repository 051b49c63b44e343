"""ALSFactorizationModel without a GPU: constructor and keyword validation, the device CSR builders (stock tensor ops, here on
CPU tensors) against scipy.sparse, and the model-level checks of tests/als_checks.py through the emulator build of the kernels.
The same model-level checks run on the gfx950 library in tests/test_gpu_als.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import als_checks as ac
from emu_backend import emu_lib
from spotlight_amd import _native
from spotlight_amd.factorization import als
from spotlight_amd.factorization import implicit as host
from spotlight_amd.factorization.als import ALSFactorizationModel
from spotlight_amd.interactions import Interactions


@pytest.fixture()
def emu_device(monkeypatch):
    eng = _native.Engine(0, lib=emu_lib())
    monkeypatch.setattr(host, '_engine_for', lambda device: eng)
    monkeypatch.setattr(host, '_stream_for', lambda device: 0)
    monkeypatch.setattr(host, '_model_device', lambda: torch.device('cpu'))
    yield eng
    eng.close()


def test_importable_through_the_reference_paths():
    from spotlight.factorization.als import ALSFactorizationModel as aliased
    assert aliased is ALSFactorizationModel
    assert issubclass(ALSFactorizationModel, host.ImplicitFactorizationModel)


def test_constructor_defaults_and_seed_flow():
    model = ALSFactorizationModel(random_state=np.random.RandomState(7))
    assert (model._embedding_dim, model._n_iter, model._regularization, model._alpha, model._use_weights) == (32, 15, 0.01, 40.0, False)
    assert model.loss_history_ == [] and model._net is None
    # the constructor consumes the stream exactly as the parent's does
    parent = host.ImplicitFactorizationModel(random_state=np.random.RandomState(7))
    a, b = model._random_state.get_state(), parent._random_state.get_state()
    assert (a[1] == b[1]).all() and a[2] == b[2]


@pytest.mark.parametrize('kw', [dict(loss='bpr'), dict(batch_size=128), dict(l2=0.1), dict(learning_rate=0.1), dict(optimizer_func=None),
                                dict(sparse=True), dict(num_negative_samples=3), dict(negative_sampling='popularity'),
                                dict(negative_sampling_power=0.5), dict(verify_negatives=True), dict(verify_tries=2), dict(nonsense=1)])
def test_keywords_without_a_meaning_are_refused(kw):
    rs = np.random.RandomState(3)
    state = rs.get_state()
    with pytest.raises(TypeError, match=list(kw)[0]):
        ALSFactorizationModel(random_state=rs, **kw)
    after = rs.get_state()
    assert (after[1] == state[1]).all() and after[2] == state[2], 'a refused constructor consumed the RandomState'


@pytest.mark.parametrize('kw', [dict(embedding_dim=0), dict(embedding_dim=129), dict(embedding_dim=70), dict(embedding_dim=256),
                                dict(regularization=-1.0), dict(regularization=float('nan')), dict(alpha=0.0), dict(alpha=float('inf')),
                                dict(n_iter=-1)])
def test_bad_values_are_refused(kw):
    with pytest.raises(ValueError, match=list(kw)[0]):
        ALSFactorizationModel(**kw)


def test_unsupported_representations_are_refused():
    from spotlight_amd.factorization.representations import BilinearNet
    from spotlight_amd.layers import BloomEmbedding
    bloom = lambda n: BloomEmbedding(n, 16, compression_ratio=0.5, num_hash_functions=2)
    for net in (BilinearNet(20, 30, 16, user_embedding_layer=bloom(20)), BilinearNet(20, 30, 16, item_embedding_layer=bloom(30))):
        with pytest.raises(ValueError, match='BloomEmbedding'):
            ALSFactorizationModel(embedding_dim=16, representation=net)
    with pytest.raises(NotImplementedError, match='custom representation'):
        ALSFactorizationModel(representation=torch.nn.Linear(3, 3))
    ALSFactorizationModel(embedding_dim=16, representation=BilinearNet(20, 30, 16))  # a plain BilinearNet is the usual net


def test_weights_are_validated_before_anything_runs(emu_device):
    ids = np.array([0, 1, 2], np.int32)
    for weights, err in ((None, 'needs interactions.weights'), (np.array([1.0, 0.0, 2.0], np.float32), 'strictly positive'),
                         (np.array([1.0, np.inf, 2.0], np.float32), 'finite')):
        model = ALSFactorizationModel(embedding_dim=8, use_weights=True, random_state=np.random.RandomState(1))
        with pytest.raises(ValueError, match=err):
            model.fit(Interactions(ids, ids, weights=weights, num_users=3, num_items=3))
        assert model._net is None, 'the tables were allocated before the weights were checked'


@pytest.mark.parametrize('weighted', [False, True])
def test_csr_builders_against_scipy(weighted):
    rs = np.random.RandomState(11)
    U, I, n, alpha = 37, 23, 900, 2.5  # 900 pairs over 851 cells: plenty of duplicates, several of multiplicity > 2
    users, items = rs.randint(0, U, n), rs.randint(0, I, n)
    users[:6], items[:6] = 5, 9  # one pair six times
    weights = rs.uniform(0.1, 3.0, n).astype(np.float32) if weighted else None
    by_user, by_item = als.build_csrs(users, items, weights, U, I, alpha, torch.device('cpu'))
    data = weights.astype(np.float64) if weighted else np.ones(n)
    for csr, want in ((by_user, sp.coo_matrix((data, (users, items)), shape=(U, I)).tocsr()),
                      (by_item, sp.coo_matrix((data, (items, users)), shape=(I, U)).tocsr())):
        want.sum_duplicates()
        want.sort_indices()
        assert csr.off.dtype == csr.cols.dtype == torch.int64 and csr.vals.dtype == torch.float32
        assert np.array_equal(csr.off.numpy(), want.indptr) and np.array_equal(csr.cols.numpy(), want.indices)
        assert csr.nnz == want.nnz and csr.n_rows == want.shape[0]
        if weighted:  # scipy adds the duplicates in its own order: equal to float64 rounding, then rounded to float32
            np.testing.assert_allclose(csr.vals.numpy(), (alpha * want.data).astype(np.float32), rtol=2e-7)
        else:
            assert ac.same_bits(csr.vals.numpy(), (alpha * want.data).astype(np.float32))
    # the two sides hold the same entries
    a = sp.csr_matrix((by_user.vals.numpy(), by_user.cols.numpy(), by_user.off.numpy()), shape=(U, I))
    b = sp.csr_matrix((by_item.vals.numpy(), by_item.cols.numpy(), by_item.off.numpy()), shape=(I, U))
    assert (a != b.T).nnz == 0
    # the restatement's builder (tests/als_checks.py) agrees
    off, cols, r = ac.merge_duplicates(users, items, data, U)
    assert np.array_equal(off, by_user.off.numpy()) and np.array_equal(cols, by_user.cols.numpy())


def test_csr_builders_without_interactions():
    by_user, by_item = als.build_csrs(np.zeros(0, np.int32), np.zeros(0, np.int32), None, 4, 3, 1.0, torch.device('cpu'))
    assert by_user.off.tolist() == [0] * 5 and by_item.off.tolist() == [0] * 4 and by_user.nnz == by_item.nnz == 0
    assert by_user.cols.numel() == 1 and by_user.vals.numel() == 1  # never a NULL address


# ---- model level, through the emulator build ------------------------------------------------------------------------------------------
def test_fit_against_the_float64_restatement(emu_device):
    ac.check_model_fit_against_float64()


def test_determinism_and_weights(emu_device):
    ac.check_model_determinism_and_weights()


def test_fold_in_recommend_evaluation_pickle(emu_device):
    ac.check_model_serving()


def test_a_representation_of_another_dim_than_the_keyword(emu_device):
    ac.check_model_representation_dim_wins()


def test_failed_rows_and_open_scopes(emu_device):
    ac.check_model_failure_and_scope(emu_device)
