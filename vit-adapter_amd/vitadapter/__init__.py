"""vitadapter -- MI355X-native ViT-Adapter backbone (host side).

``vitadapter.backbones.ViTAdapter`` has the constructor signature, forward contract and
state_dict layout of the reference's two ``ViTAdapter`` classes
(/root/reference/segmentation/mmseg_custom/models/backbones/vit_adapter.py:19-137 and
/root/reference/detection/mmdet_custom/models/backbones/vit_adapter.py:19-132); the deformable
attention inside it runs on the hand-written gfx950 kernels of libvitadapter_hip.so.
"""
from .backbones import (BEiTAdapter, ViTAdapter, ViTAdapterDet, ViTAdapterSeg, register_backbones,
                        register_beit_adapter)

from .mmcv_attention import MultiScaleDeformableAttention, register_attention
from .pixel_decoder import MSDeformAttnPixelDecoder, register_pixel_decoder
from .mask2former_head import Mask2FormerHead
from .segmentor import EncoderDecoder, EncoderDecoderMask2Former, EncoderDecoderMask2FormerAug
from .evaluation import (SegEvaluator, eval_metrics, intersect_and_union, mean_dice, mean_fscore, mean_iou, pre_eval_to_metrics,
                         total_area_to_metrics, total_intersect_and_union)
from .pipelines import ToMask

__all__ = ['ViTAdapter', 'ViTAdapterSeg', 'ViTAdapterDet', 'register_backbones', 'BEiTAdapter',
           'register_beit_adapter',
           'MultiScaleDeformableAttention', 'register_attention', 'MSDeformAttnPixelDecoder', 'register_pixel_decoder',
           'Mask2FormerHead', 'EncoderDecoderMask2Former', 'EncoderDecoderMask2FormerAug', 'EncoderDecoder',
           'SegEvaluator', 'intersect_and_union', 'total_intersect_and_union', 'total_area_to_metrics', 'pre_eval_to_metrics',
           'eval_metrics', 'mean_iou', 'mean_dice', 'mean_fscore', 'ToMask']
