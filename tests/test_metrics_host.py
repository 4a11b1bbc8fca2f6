"""The Keras 'accuracy' metric on the host: utility.categorical_accuracy (the NumPy mirror every device count is held to) on
hand-made rows, and the parts of the model surface that need no device - metrics_names, evaluate before compile,
fit_generator on every model."""
import numpy as np
import pytest

from longterm360fov_amd import utility as U

NAN = np.nan


def acc(pred, target):
    return U.categorical_accuracy(np.asarray(pred, np.float32), np.asarray(target, np.float32))


def test_ties_take_the_lowest_index():
    # pred's maxima at (1, 2) -> 1; at (0, 3) -> 0; all equal -> 0
    pred = [[0, 2, 2, 1], [5, 1, 1, 5], [3, 3, 3, 3]]
    assert acc(pred, [[0, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]]) == (3, 3)
    assert acc(pred, [[0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 1]]) == (0, 3)
    # ties in the target as well: (2, 3) -> 2
    assert acc([[0, 0, 1, 0]], [[0, 0, 7, 7]]) == (1, 1)


def test_signed_zeros_are_equal():
    # -0.0 then +0.0 is a tie: index 0, not the +0.0
    assert acc([[-0.0, 0.0, -0.0]], [[1, 0, 0]]) == (1, 1)
    assert acc([[-0.0, 0.0, -0.0]], [[0, 1, 0]]) == (0, 1)
    assert acc([[-1.0, -0.0, 0.0]], [[0, 1, 0]]) == (1, 1)


def test_the_first_nan_is_the_maximum():
    assert acc([[1, NAN, 9, NAN]], [[0, 1, 0, 0]]) == (1, 1)
    assert acc([[1, NAN, 9, NAN]], [[0, 0, 1, 0]]) == (0, 1)
    # in the target too
    assert acc([[0, 0, 0, 1]], [[0, 5, 1, NAN]]) == (1, 1)
    assert acc([[NAN, NAN]], [[NAN, 1]]) == (1, 1)


def test_an_all_zero_target_row_has_argmax_zero():
    """The common row of a heat map that is one-hot over its pixels: no frame looks at this pixel."""
    tgt = np.zeros((3, 5), np.float32)
    assert acc([[9, 0, 0, 0, 0], [0, 0, 0, 0, 9], [0.2, 0.2, 0.2, 0.2, 0.2]], tgt) == (2, 3)


def test_one_channel_is_binary_accuracy_rounding_half_to_even():
    pred = [[0.5], [1.5], [2.5], [-0.5]]
    assert acc(pred, [[0], [2], [2], [-0.0]]) == (4, 4)
    assert acc(pred, [[1], [1], [3], [-1]]) == (0, 4)
    assert acc([[NAN], [0.4]], [[NAN], [0]]) == (1, 2)
    # every element is a row: (2, 3, 1) counts six
    assert acc(np.full((2, 3, 1), 0.9), np.ones((2, 3, 1))) == (6, 6)


def test_shapes():
    rng = np.random.default_rng(0)
    p = rng.normal(size=(3, 4, 5, 6))
    assert U.categorical_accuracy(p, p) == (60, 60)
    assert U.categorical_accuracy(np.zeros((0, 6)), np.zeros((0, 6))) == (0, 0)
    with pytest.raises(ValueError):
        U.categorical_accuracy(np.zeros((2, 6)), np.zeros((2, 5)))


def _models():
    from longterm360fov_amd import models as M
    from oracle import fov_oracle as O
    yield M.Seq2SeqLSTM(latent_dim=32, seed=1)
    yield M.OthersMixingSeq2Seq(latent_dim=32, num_user=4, seed=1)
    yield M.KerasSingleLSTM(latent_dim=32, seed=1)
    yield M.ConvLSTMSeq2Seq(O.init_convlstm_seq2seq(1, C=10, latent_dim=8, k=3, head="conv2d", head_filters=(24, 40)))


def test_metrics_names():
    for m in _models():
        assert m.metrics_names == ["loss"]
        for metrics, names in ((None, ["loss"]), (["accuracy"], ["loss", "acc"]), (["acc"], ["loss", "acc"]), (["mae"], ["loss"])):
            m.compile(metrics=metrics)
            assert m.metrics_names == names
            assert m.metrics == list(metrics or [])      # kept as given, an unknown name raises nothing


def test_evaluate_before_compile_raises_without_a_device():
    x = y = np.zeros((2, 2, 6), np.float32)
    for m in _models():
        for call in (lambda: m.evaluate(x, y), lambda: m.test_on_batch(x, y), lambda: m.evaluate_generator(iter([(x, y)]), 1),
                     lambda: m.fit_generator(iter([(x, y)]), 1)):
            with pytest.raises(RuntimeError, match="compile"):
                call()
        assert m._trainer is None


def test_every_model_has_the_generator_surface():
    from longterm360fov_amd import models as M
    for cls in (M.ConvLSTMSeq2Seq, M.Seq2SeqLSTM, M.OthersMixingSeq2Seq, M.StackedSeq2SeqLSTM, M.KerasSingleLSTM):
        for name in ("fit_generator", "evaluate_generator", "evaluate", "test_on_batch"):
            assert callable(getattr(cls, name))
    assert M.OthersMixingSeq2Seq.fit_generator is M.KerasModelSurface.fit_generator
