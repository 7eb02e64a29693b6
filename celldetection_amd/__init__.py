"""celldetection_amd -- MI355X-native (gfx950, HIP) Contour Proposal Network inference path.

Drop-in for the CPN inference path of FZJ-INM1-BDA/celldetection: ``models.Cpn*`` / ``models.CPN``,
``fetch_model`` / ``load_model`` (reference file format), ``ops`` (decode / NMS) and the tiled slide inference
loop.  Everything computes in hand-written HIP kernels behind the C ABI of ``libcpn_hip.so``
(``include/cpn_hip.h``); there is no CPU fallback.
"""
from . import cpn as models  # ``cd.models.CpnResNeXt101UNet`` -> ``celldetection_amd.models.CpnResNeXt101UNet``
from . import (augment, components, flat_labels, fourier, h5, inference, instance_eval, label_contours, labels, nn, objective, ops, optim, overlay, preprocess, region_props, shape_props, synth,
               targets, util)
from .augment import RandomAffine
from .components import (fill_label_gaps_, label_components, masks2labels, relabel_, remove_partials_, rgb_to_scalar, stack_labels,
                         unary_masks2labels)
from .flat_labels import resolve_label_channels
from .fourier import contours2fourier, efd, labels2fourier
from .h5 import from_h5, to_h5
from .instance_eval import LabelMatcher, LabelMatcherList
from .objective import CPNObjective, collate_cpn_targets
from .optim import AdamW, clip_grad_norm_, grad_norm, step_info
from .region_props import labels2property_table, region_properties
from .shape_props import shape_properties
from .label_contours import labels2contour_list as labels2contours  # ``cd.data.labels2contours`` is that function
from .label_contours import resample_contours
from .labels import contours2labels
from .overlay import contours2overlay, label_cmap, random_colors_hsv
from .targets import CPNTargetGenerator, filter_instances_, labels2distances, mask_labels_by_distance_
from .util import (dict2model, fetch_model, get_tiling_slices, load_model, model2dict, save_fetchable_model)

__version__ = '0.1.0'
__all__ = ['models', 'ops', 'util', 'synth', 'inference', 'labels', 'contours2labels', 'preprocess', 'h5', 'to_h5', 'from_h5', 'fetch_model', 'load_model', 'save_fetchable_model', 'dict2model',
           'model2dict', 'get_tiling_slices', 'instance_eval', 'LabelMatcher', 'LabelMatcherList', 'flat_labels',
           'resolve_label_channels', 'region_props', 'region_properties', 'labels2property_table', 'shape_props', 'shape_properties', 'overlay', 'contours2overlay',
           'label_cmap', 'random_colors_hsv', 'label_contours', 'labels2contours', 'resample_contours', 'fourier', 'efd', 'contours2fourier',
           'labels2fourier', 'targets', 'labels2distances', 'mask_labels_by_distance_', 'filter_instances_', 'CPNTargetGenerator',
           'objective', 'CPNObjective', 'collate_cpn_targets', 'components', 'label_components', 'relabel_', 'stack_labels',
           'rgb_to_scalar', 'unary_masks2labels', 'masks2labels', 'fill_label_gaps_', 'remove_partials_', 'nn',
           'optim', 'AdamW', 'clip_grad_norm_', 'grad_norm', 'step_info', 'augment', 'RandomAffine']
