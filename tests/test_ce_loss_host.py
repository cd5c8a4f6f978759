"""The softmax cross-entropy 1-vs-all loss, what can be said without a GPU: the export, the refusal of CPU tensors,
the configuration field and the driver's choice of loss."""
import pytest
import torch


def test_ce_loss_is_exported():
    import r_tucker_amd as rt
    from r_tucker_amd import ops
    assert rt.ce_loss_1vN is ops.ce_loss_1vN


@pytest.mark.parametrize("matrix_free", [False, True])
def test_cpu_tensors_are_refused(matrix_free):
    import r_tucker_amd as rt
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.ce_loss_1vN(torch.zeros(2, 4, 4), torch.zeros(4, 2), torch.zeros(5, 4), torch.zeros(5, 4), torch.tensor([0]),
                       torch.tensor([0]), None, torch.tensor([0]), label_smoothing=0.1, matrix_free=matrix_free)


def test_train_config_loss_defaults_to_bce():
    from configs.base_config import NAMED_CONFIGS, TrainConfig
    assert TrainConfig().loss == "bce"
    assert all(make().train_cfg.loss == "bce" for make in NAMED_CONFIGS.values())


def test_batch_loss_fn_rejects_an_unknown_loss():
    import r_tucker_amd as rt
    from r_tucker_amd import driver
    model = rt.AsymmetricR_TuckER((50, 4), (3, 4, 4), device="cpu")
    with pytest.raises(ValueError, match="unknown loss"):
        driver.batch_loss_fn(model, torch.tensor([0]), torch.tensor([0]), None, torch.tensor([0]), 0.1, 1e-4, loss="hinge")
    for name in ("bce", "ce"):
        assert callable(driver.batch_loss_fn(model, torch.tensor([0]), torch.tensor([0]), None, torch.tensor([0]), 0.1, 1e-4,
                                             loss=name))
