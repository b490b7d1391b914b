from .architectures import HigherHRNet
from .grouping import MPPEHeatmapParser
from .model import InferenceKeypointsModel, KeypointsModel, KeypointsModule
from .results import InferenceKeypointsResult, KeypointsResult

__all__ = ["HigherHRNet", "MPPEHeatmapParser", "InferenceKeypointsModel", "InferenceKeypointsResult", "KeypointsModel", "KeypointsModule"]
from .loss import AEGroupingLoss, AEKeypointsLoss, HeatmapsLoss
from . import coco_eval, crowd_mask, evaluation, targets, tracking
from .crowd_mask import CrowdSegments, crowd_masks, get_crowd_mask, raw_sample
from .train_input import Mosaic, TrainInput, mosaic_joints
from .tracking import PoseTracker
from . import jpeg
from .jpeg import JpegImage, JpegIndexCache, MJPEGReader, MJPEGWriter, build_jpeg_index, decode_jpeg_device, encode_jpeg_device, jpeg_info, load_jpeg, save_jpeg
from .visualization import DEFAULT_PALETTE, build_primitives, jet_lut, plot_connections, plot_heatmaps
from . import text
from .text import layout_put_txt, load_font, put_txt, put_txt_device, put_txt_host, text_size, video_labels
from . import sample_plot
from .sample_plot import plot_examples, plot_examples_jpeg, plot_raw, plot_sample, plot_segmentations, seg_tables
from . import pose_score
from .pose_score import image_OKS, image_PCKh, match_preds_to_targets, object_OKS, object_PCKh, pack_targets
