from .metrics_calculator import MetricsCalculator

__all__ = ["MetricsCalculator"]
