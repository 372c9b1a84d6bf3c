"""examples/catheter_geofno.py (the port of the reference's Geo-FNO catheter example) at reduced sizes: it trains, evaluates and
writes its figures, and the validator's L2Rel after training is below the untrained model's."""
import os

import numpy as np

from tests.common import make_dev_fixture

dev = make_dev_fixture()


def test_catheter_example_trains_evaluates_and_plots(dev, tmp_path):
    from examples import catheter_geofno as ex

    cfg = dict(ex.DEFAULTS, output_dir=str(tmp_path), width=16, modes=8, padding=10, s=101, output_np=101, n_train=40, n_test=12,
               batch_size=10, epochs=6, step_size=4, eval_during_train=False, save_freq=0, log_freq=1, learning_rate=0.005)
    inputs, labels, para = ex.getdata(5, 101, 0)
    assert inputs.shape == (5, 101, 2) and labels.shape == (5, 101, 1) and para.shape == (4, 5)
    assert inputs.dtype == np.float32 and np.isfinite(labels).all()
    solver = ex.build(cfg)
    untrained, _ = solver.eval()
    before = solver.model.flat_params.cpu().numpy().copy()
    solver.train()
    solver.plot_loss_history(by_epoch=True, smooth_step=1)
    assert np.isfinite(solver.last_losses["loss"])
    after = solver.model.flat_params.cpu().numpy()
    assert np.isfinite(after).all() and np.abs(after - before).max() > 0
    trained, group = solver.eval()
    l2 = group["validator1"]["L2Rel.output"]
    print(f"validator L2Rel: untrained {untrained:.4f} -> trained {trained:.4f}")
    assert np.isfinite(trained) and np.isfinite(l2) and trained < untrained
    errors, paths = ex.evaluate(cfg, solver.model)
    assert len(errors) == 2 and all(np.isfinite(e) for e in errors)
    assert all(os.path.getsize(p) > 0 for p in paths)
    assert any(f.endswith(".png") or f.endswith(".jpg") for _, _, fs in os.walk(str(tmp_path)) for f in fs)  # the loss history
    # predict goes through the same executor; the training step's buffer set survived evaluation at other batch sizes
    pred = solver.predict({"input": inputs}, batch_size=5)["output"]
    assert tuple(pred.shape) == (5, 101, 1)
    assert solver.model.native().generation == 0
    for fn in (ex.export, ex.inference):
        try:
            fn(cfg)
        except NotImplementedError:
            continue
        raise AssertionError("export / inference are out of scope and must raise")
