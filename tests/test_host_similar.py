"""similar_items() / similar_users() of the models through the emulator build of the kernels (no GPU), and of the row-sharded
model over gloo at world 2 and 3 (tests/shard_neighbors_worker.py).  The same checks run on the gfx950 library in
tests/test_gpu_similar.py."""
import os

import pytest
import torch

import similar_checks as sc
from emu_backend import emu_lib
from spotlight_amd import _native
from spotlight_amd.factorization import implicit as host
from test_sharded import run_world

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, 'shard_neighbors_worker.py')


@pytest.fixture()
def emu_device(monkeypatch):
    eng = _native.Engine(0, lib=emu_lib())
    monkeypatch.setattr(host, '_engine_for', lambda device: eng)
    monkeypatch.setattr(host, '_stream_for', lambda device: 0)
    monkeypatch.setattr(host, '_model_device', lambda: torch.device('cpu'))
    yield eng
    eng.close()


def test_implicit_model(emu_device):
    sc.check_factorization()


def test_explicit_model(emu_device):
    sc.check_factorization(cls=sc.ExplicitFactorizationModel, loss='regression')


def test_ties_in_the_model(emu_device):
    sc.check_ties_in_the_model()


def test_bloom_item_table(emu_device):
    sc.check_bloom_item_table()


def test_custom_representation_is_refused(emu_device):
    sc.check_custom_representation()


def test_sequence_model_never_returns_the_padding_item(emu_device):
    sc.check_sequence_model()


def test_refused_inside_a_fit_scope(emu_device):
    sc.check_refused_inside_a_fit_scope(emu_device, 0)


@pytest.mark.parametrize('world,items', [(2, 47), (3, 47), (3, 2)])  # (3, 2): a world larger than the number of items
def test_sharded_similar_items_matches_single_device_model(world, items):
    run_world(world, [items], worker=WORKER, token='SHARD_NEIGHBORS_OK', timeout=240)
