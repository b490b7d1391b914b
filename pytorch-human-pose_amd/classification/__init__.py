from .input import ClsInput, CropParams, CropWindow, inference_geometry, random_resized_crop_params
from .loss import ClassificationLoss
from .model import ClassificationModel, InferenceClassificationModel, InferenceClassificationResult
from .module import ClassificationModule, ClassificationResult

__all__ = ["ClassificationLoss", "ClassificationModel", "ClassificationModule", "ClassificationResult", "ClsInput", "CropParams", "CropWindow",
           "InferenceClassificationModel", "InferenceClassificationResult", "inference_geometry", "random_resized_crop_params"]
