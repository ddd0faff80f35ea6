"""abnet3_amd: MI355X-native implementation of bootphon/abnet3's Siamese
training hot path (SiameseNetwork forward/backward, coscos2/cosmargin, DTW
frame alignment, filterbanks) behind the reference's own class surfaces.

Submodules mirror the reference's module names so that the class-name lookup
of abnet3/gridsearch.py:145-202 resolves against this package unchanged:
    abnet3_amd.model, .loss, .trainer, .embedder, .dataloader, .features, .utils
"""
__version__ = '0.1.0'


def __getattr__(name):
    # `from abnet3_amd import KMeansQuantizer`, without importing torch when the package alone is imported
    if name == 'KMeansQuantizer':
        from .kmeans import KMeansQuantizer
        return KMeansQuantizer
    if name in ('StickyHmmPosteriorgram', 'TransitionHmmPosteriorgram'):
        from . import hmm
        return getattr(hmm, name)
    if name in ('TermEvaluator', 'edit_distance_batch', 'read_alignment', 'read_classes', 'transcribe'):
        from . import tde
        return getattr(tde, name)
    if name in ('TermPrefilter', 'lsh_planes', 'lsh_signatures', 'diag_hits_batch'):
        from . import prefilter
        return getattr(prefilter, name)
    if name in ('SameDifferentEvaluator', 'scores_from_histogram', 'pair_histogram'):
        from . import samediff
        return getattr(samediff, name)
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
