"""The surface of the reference's ``evolvegcn_functions`` in one module:

    import tmgcn_amd.ef as ef            # instead of: import evolvegcn_functions as ef

is the only edit a reference EvolveGCN script needs (experiment_*_evolvegcn*.py, graph_SEIR_evolvegcn.py; the link
prediction scripts also import ``embedding_help_functions``: tmgcn_amd.ehf).  ``EvolveGCN_1_layer``,
``EvolveGCN_2_layer`` and ``EvolveGCN_reg`` are the classes of tmgcn_amd.evolvegcn (the weight evolution runs in
csrc/evolvegcn.hip) with ``host_operands`` set, as in tmgcn_amd.ehf: the logits stay on the MI355X as
``hosted.DeviceResult`` and pull the host tensors a script combines them with (targets, class weights, ``argmax``) over
to the device.  The returned W are plain fp64 device tensors that go back in as ``W_init``.
"""
from . import evolvegcn as _evolvegcn


class EvolveGCN_1_layer(_evolvegcn.EvolveGCN_1_layer):
    host_operands = True


class EvolveGCN_2_layer(_evolvegcn.EvolveGCN_2_layer):
    host_operands = True


class EvolveGCN_reg(_evolvegcn.EvolveGCN_reg):
    host_operands = True


for _c in (EvolveGCN_1_layer, EvolveGCN_2_layer, EvolveGCN_reg):
    _c.__doc__ = getattr(_evolvegcn, _c.__name__).__doc__
del _c
