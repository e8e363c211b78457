"""fp64 restatement, in numpy only, of the reference's validation loops (graphphysics/training/lightning_module.py):
``_make_prediction`` (:375-409), the metrics of ``validation_step`` (:411-456) and ``on_validation_epoch_end`` (:467-492),
on top of the Simulator restatement of tests/sim_reference.py.  Written from the reference's text, independent of the engine.

The network is a callable ``net(node_features, edge_features) -> [N, O]`` on the NORMALISED inputs (what the Simulator hands
to its model), so a test chooses how much of a model the fp64 side carries: an affine map, or the oracle in double precision.

What it pins down:
  * the previous-data feedback is ``predicted_outputs - current_output`` taken AFTER ``predicted_outputs[mask] = target[mask]``
    (:398-401), where ``current_output`` are the output columns of the frame the model saw, i.e. with the last prediction
    written in (:380-392);
  * the first frame of a trajectory is used as it is (``last_prediction is None``, :378);
  * ``val_loss`` is the masked L2 over the rows whose type is in ``masks`` (:443-449, utils/loss.py:70-75), logged per step
    and averaged over the steps of the epoch;
  * ``val_1step_rmse`` is the mean over the trajectories of ``sqrt(mean (pred - target)^2)`` of their first frame (:452-455,
    :485-489);
  * ``val_all_rollout_rmse`` is ``sqrt(mean)`` over the CONCATENATION of all frames (:469-474): frames weigh by their rows.
"""
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

import sim_reference as SR


class Rollout64:
    def __init__(self, sim: SR.Simulator64, net: Callable, use_previous_data: bool = False,
                 previous: Tuple[Optional[int], Optional[int]] = (None, None),
                 masks: Sequence[float] = (SR.NODE_NORMAL, SR.NODE_OUTFLOW)):
        self.sim, self.net = sim, net
        self.use_previous_data, self.previous, self.masks = use_previous_data, previous, tuple(float(m) for m in masks)

    # lightning_module.py:375-409
    def make_prediction(self, x, y, edge_attr, last_prediction, last_previous_data):
        lay = self.sim.lay
        x = np.array(x, dtype=np.float64)                                        # batch.clone(), :376
        if last_prediction is not None:                                          # :378
            x[:, lay.out_start:lay.out_end] = last_prediction                    # :380-382
            if self.use_previous_data:
                x[:, self.previous[0]:self.previous[1]] = last_previous_data     # :383-386
        keep = SR.keep_mask(x[:, lay.type_idx])                                  # build_mask, :27-35 (mask = not keep)
        target = np.asarray(y, dtype=np.float64)[:, :lay.O]                      # :388
        current_output = x[:, lay.out_start:lay.out_end].copy()                  # :390-392
        xn, _, en = self.sim.build_input(x, y, edge_attr, training=False)        # self.model(batch) in eval mode, :394-395
        predicted = self.sim.build_outputs(x, self.net(xn, en))
        predicted = np.where(keep[:, None], predicted, target)                   # :398
        last_prediction = predicted                                              # :399
        if self.use_previous_data:
            last_previous_data = predicted - current_output                      # :400-401
        return x, predicted, target, last_prediction, last_previous_data

    def rollout(self, frames):
        """frames: (x, y, edge_attr) per step; the predictions and the frames the model saw"""
        last = prev = None
        preds, seen = [], []
        for x, y, ea in frames:
            xb, pred, _, last, prev = self.make_prediction(x, y, ea, last, prev)
            preds.append(pred)
            seen.append(xb)
        return preds, seen

    # validation_step :439-456
    def frame_metrics(self, x_seen, predicted, target):
        lay = self.sim.lay
        d2 = (np.asarray(predicted, dtype=np.float64) - np.asarray(target, dtype=np.float64)[:, :lay.O]) ** 2
        w = np.isin(np.asarray(x_seen)[:, lay.type_idx].astype(np.float64), self.masks)   # loss.py:70-75: rows whose type is a mask
        return dict(S_all=float(d2.sum()), S_loss=float(d2[w].sum()), n_loss=float(w.sum()), N=float(d2.shape[0]),
                    val_loss=float(d2[w].mean()) if w.any() else float("nan"),
                    rmse=float(np.sqrt(d2.mean())) if d2.size else float("nan"))

    # validation_step over every frame + on_validation_epoch_end :467-492
    def validate(self, trajectories):
        outputs, targets, losses, first, predictions = [], [], [], [], []
        for frames in trajectories:                                              # _reset_validation_trajectory, :370-373
            last = prev = None
            preds = []
            for step, (x, y, ea) in enumerate(frames):
                xb, pred, target, last, prev = self.make_prediction(x, y, ea, last, prev)
                m = self.frame_metrics(xb, pred, target)
                outputs.append(pred)                                             # :441-442
                targets.append(target)
                losses.append(m["val_loss"])                                     # :443-449
                if step == 0:
                    first.append(m["rmse"])                                      # :452-455
                preds.append(pred)
            predictions.append(preds)
        return dict(val_loss=float(np.mean(losses)), val_loss_per_step=np.array(losses),
                    val_all_rollout_rmse=metrics_from_predictions(outputs, targets)["val_all_rollout_rmse"],
                    val_1step_rmse=float(np.mean(first)), predictions=predictions)


def metrics_from_predictions(predicteds, targets):
    """on_validation_epoch_end's concatenate-then-mean (:469-474), in fp64, from any list of per-frame arrays"""
    p = np.concatenate([np.asarray(a, dtype=np.float64) for a in predicteds], axis=0)
    t = np.concatenate([np.asarray(a, dtype=np.float64) for a in targets], axis=0)
    return dict(val_all_rollout_rmse=float(np.sqrt(((p - t) ** 2).mean())))
