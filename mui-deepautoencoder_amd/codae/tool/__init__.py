"""codae.tool: the names the training scripts import (same public surface as the reference package, so that
`from codae.tool import Corrupter, CombinedCriterion, ...` resolves here), gathered from this build's modules.
The reference's legacy argparse table (codae/tool/parser.py) and attr-dict (dictionnary.py) are out of scope
(SURVEY.md section 2): nothing on the path uses them, so they have no counterpart here."""
from . import average, batching, clusters, codes, compat, contrast, corruption, criteria, dropout, emphasis, noise, norm, optimizer, presence, recon_loss, residual, runlog, sparse, tied, variable_loss

_PUBLIC = {
    runlog: ("set_logging", "display_info", "get_date", "PlotDrawer", "export_parameters_to_json"),
    batching: ("collate_embedding", "simple_collate", "load_dataset_of_embeddings", "Normalizer",
               "get_mask_transformation"),
    corruption: ("Corrupter",),
    noise: ("InputNoise",),        # not in the reference: the DAE noise models its whole-slot blank leaves out
    emphasis: ("LossEmphasis",),   # not in the reference either: the loss half of the same paper (its section 4.3)
    recon_loss: ("ReconstructionLoss",),   # the training criterion of the fused step: MSE, L1, SmoothL1, Huber, per-slot cosine
    # the mixed-variable (tabular) criterion of the fused step: RMSE per numeric variable, NLL per one-hot variable
    variable_loss: ("VariableLoss",),
    contrast: ("SlotContrast",),   # a sampled softmax against the slot's other items, on top of the criterion: trains the ranking
    presence: ("SlotPresence",),   # rows that lack an item in some slots: absent slots stay out of input, loss and inventory
    dropout: ("HiddenDropout",),   # torch users expect Dropout between the Linears: the fused step's form of it
    norm: ("Norm", "norm_from_config"),   # parameter-free layer / RMS normalisation of hidden outputs, per batch row, in every forward
    # the k-sparse autoencoder's hard top-k code layer: the `keep` largest-magnitude units of the code per row, in every forward
    sparse: ("SparseCode", "sparse_from_config"),
    residual: ("Residual", "residual_from_config"),   # identity skips around equal-width hidden layers, in every forward
    optimizer: ("Optimizer", "LRSchedule", "optimizer_from_config"),   # what the update does: AdamW / SGD / AMSGrad, lr schedule
    average: ("WeightAverage", "weight_average_from_config"),   # an EMA / SWA of the iterates kept by the update, for evaluation
    tied: ("TiedWeights",),        # the decoder uses the encoder's transposed matrices: pairs, and the fold / mirror in torch ops
    criteria: ("get_rmse", "RankingLoss", "ComplementRetriever", "RetrievalMetrics", "retrieval_metrics_from_config",
               "CombinedCriterion"),
    # outfits assembled per (query, slot) from the items of different rows: their score, and the AUC of real against swapped ones
    compat: ("Compatibility", "CompatibilityMetrics", "compatibility_from_config"),
    # the latent vector of an outfit and nearest neighbours in code space: "which outfits look like this one?"
    codes: ("OutfitCodes", "codes_from_config"),
    # spherical k-means over a bank of codes: "which kinds of outfit are there, and to which does this one belong?"
    clusters: ("CodeClusters", "clusters_from_config"),
}
__all__ = []
for _module, _names in _PUBLIC.items():
    for _name in _names:
        globals()[_name] = getattr(_module, _name)
        __all__.append(_name)
del _module, _names, _name
