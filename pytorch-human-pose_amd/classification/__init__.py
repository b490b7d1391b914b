from .evaluation import ClsEvaluator, ClsTopK, evaluate_images, image_folder_items, score_logits
from .input import ClsInput, CropParams, CropWindow, inference_geometry, random_resized_crop_params
from .loss import ClassificationLoss
from .model import ClassificationModel, InferenceClassificationModel, InferenceClassificationResult
from .module import ClassificationModule, ClassificationResult
from .visualization import plot_top_preds, plot_top_preds_batch

__all__ = ["ClassificationLoss", "ClassificationModel", "ClassificationModule", "ClassificationResult", "ClsEvaluator", "ClsInput", "ClsTopK", "CropParams", "CropWindow",
           "InferenceClassificationModel", "InferenceClassificationResult", "evaluate_images", "image_folder_items", "inference_geometry", "plot_top_preds", "plot_top_preds_batch", "random_resized_crop_params", "score_logits"]
