"""The surface of the reference's ``wd_gcn_functions`` in one module:

    import tmgcn_amd.wgf as wgf          # instead of: import wd_gcn_functions as wgf

is the only edit a reference WD-GCN script needs (experiment_*_wd-gcn*.py, graph_SEIR_wd_gcn.py).  ``WD_GCN`` and
``WD_GCN_reg`` are the classes of tmgcn_amd.wdgcn (the LSTM runs in csrc/wdgcn.hip, at widths beyond 8 up to 64 in
csrc/wdgcn_wide.hip) with ``host_operands`` set, as in tmgcn_amd.ehf: their outputs stay on the MI355X as ``hosted.DeviceResult`` and pull the host tensors a script combines
them with (targets, class weights, the criterion's arithmetic, ``argmax``) over to the device.
"""
from . import wdgcn as _wdgcn


class WD_GCN(_wdgcn.WD_GCN):
    host_operands = True


class WD_GCN_reg(_wdgcn.WD_GCN_reg):
    host_operands = True


for _c in (WD_GCN, WD_GCN_reg):
    _c.__doc__ = getattr(_wdgcn, _c.__name__).__doc__
del _c
