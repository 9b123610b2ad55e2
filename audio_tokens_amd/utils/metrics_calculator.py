"""The reference's utils/metrics_calculator.py on the device: the mean average precision the trainer reports after
every epoch and selects its best model by (processors/model_trainer.py:96, _save_if_best_model), and beside it the
threshold metrics that file comments out and the ROC AUC / d' AudioSet results are reported with."""
import numpy as np
import torch

from ..backend import default_backend
from ..ops import classification_metrics, mean_average_precision


class MetricsCalculator:
    @staticmethod
    def compute_metrics(predictions, labels):
        """predictions, labels: lists of per-batch [b, c] arrays (the reference's numpy arrays) or device tensors -- with
        tensors the trainer keeps its sigmoid outputs where they are and drops the .cpu().numpy().  The batches (a short
        last one included) are concatenated on the device.  -> {"mAP": float}"""
        return {"mAP": MetricsCalculator.calculate_mAP(_concat(labels), _concat(predictions))}

    @staticmethod
    def compute_all_metrics(predictions, labels, prediction_threshold=0.2):
        """The same batch lists as compute_metrics -> {"mAP", "mAUC", "d_prime", "f1_score_micro", "f1_score_macro",
        "hamming_loss"} (ops.classification_metrics: one sort per class chunk and one host read for all six;
        prediction_threshold: AudioTokensConfig.prediction_threshold, applied as predictions > threshold)."""
        return classification_metrics(_concat(labels), _concat(predictions), threshold=prediction_threshold)

    @staticmethod
    def calculate_mAP(labels, predictions):
        """Mean over the classes with a positive of sklearn's average_precision_score(labels[:, i], predictions[:, i]);
        0.0 when no class has one."""
        return mean_average_precision(labels, predictions)


def _concat(batches):
    if isinstance(batches, (np.ndarray, torch.Tensor)):
        return batches
    device = default_backend().device
    parts = [torch.from_numpy(np.ascontiguousarray(b)) if isinstance(b, np.ndarray) else b.detach() for b in batches]
    parts = [p.to(device, non_blocking=p.device.type != "cpu") for p in parts]
    dtype = parts[0].dtype
    return torch.cat([p.to(dtype) for p in parts], dim=0)
