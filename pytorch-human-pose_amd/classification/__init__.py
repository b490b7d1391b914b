from .loss import ClassificationLoss
from .model import ClassificationModel
from .module import ClassificationModule, ClassificationResult

__all__ = ["ClassificationLoss", "ClassificationModel", "ClassificationModule", "ClassificationResult"]
