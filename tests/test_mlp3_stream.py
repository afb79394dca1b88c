"""The streamed bf16 kernel of ``MLP3Energy`` on the host: the size of its weight image and the routes a CPU energy takes."""

import pytest

from torchebm_amd import _lib
from torchebm_amd.core import MLP3Energy

PIECE = 24576


@pytest.mark.parametrize("hidden,dim,pieces", [(128, 1, 5), (128, 32, 5), (128, 33, 6), (128, 64, 6), (128, 65, 8), (128, 128, 8),
                                               (64, 8, 0), (128, 0, 0), (128, 129, 0)])
def test_image_bytes(hidden, dim, pieces):
    assert _lib.lib().ebm_mlp3_image_bytes(hidden, dim) == pieces * PIECE


def test_exports_and_class_attributes():
    assert all(name in _lib._PROTOTYPES and hasattr(_lib.lib(), name) for name in _lib.EXPORTS_MLP3_STREAM)
    assert len(_lib.EXPORTS_MLP3_STREAM) == 4 and not set(_lib.EXPORTS_MLP3_STREAM) & set(_lib.EXPORTS + _lib.EXPORTS_MLP3)
    assert MLP3Energy.STREAMED_MAX_DIM == {128: 128} and MLP3Energy.streamed_bf16 is False
    assert MLP3Energy.FUSED_MAX_DIM == {64: 128, 128: 32}


@pytest.mark.parametrize("in_dim", [33, 128])
def test_fused_spec_is_none_on_cpu(in_dim):
    assert MLP3Energy(in_dim, 128).fused_spec() is None
