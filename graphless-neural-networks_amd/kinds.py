"""The one table of model families: what models.py, teacher.py, cli.py, dist.py and train_and_eval.py each used to restate about a kind.
Imports neither torch nor the library.  A new teacher family adds ONE row here (and its encoder class, its Model.__init__ branch and its
TeacherEngine.step_<kind>); every name list, refusal and dispatch below reads the row."""
from collections import namedtuple

# key: the substring of a model name that selects the family = its encoder's class name.  kind: what teacher_kind returns and every caller
# switches on.  full_graph: its training step takes the whole graph (TeacherEngine.step_<kind>).  rule, supported: the family of checks
# check_supported applies ("norm_relu", "attn", "stack" or "gcn"; None: no engine step) and the sentence it raises with.  unsharded: why
# neither sharded forward runs it (None: it is sharded).  bf16: its own bf16-inference refusal, (kernel source, document, section).
# stand_ins, global_alone: the YAML sections that stand in for a missing one of its own, in order, and whether the global section alone will do.
Kind = namedtuple("Kind", "key kind full_graph rule supported unsharded bf16 stand_ins global_alone",
                  defaults=(False, None, None, None, None, (), False))

_NORMS = "norm_type none|batch|layer and ReLU"
_HEADS = "ReLU hidden layers and a linear last layer"
_EDGES = "its edge softmax needs every in-edge of a row and "
_STEPS = "each of its K propagation steps needs the previous step's rows of the remote sources"
_LAYERS = "the previous layer's hidden rows of the remote sources"

# In the order teacher_kind must match: a key stands in front of every key it contains.
KINDS = (
    Kind("MLP", "mlp"),
    Kind("SAGE", "sage", rule="norm_relu", supported=f"SAGE with {_NORMS} (the reference's configs)"),
    Kind("GCNII", "gcnii", True, "stack", "GCNII with norm_type none and ReLU (docs/GCNII_SEMANTICS.md)",
         unsharded="each of its conv layers needs " + _LAYERS, bf16=("csrc/gcnii.hip", "docs/GCNII_SEMANTICS.md", "Out of scope")),
    Kind("GCN", "gcn", True, "gcn", "GCN with norm_type none|batch|layer"),
    Kind("APPNP", "appnp", True, "norm_relu", f"APPNP with {_NORMS} (models.py:282-344)"),
    Kind("GATv2", "gatv2", True, "attn", f"GATv2 with {_HEADS} (docs/GATV2_SEMANTICS.md)",
         unsharded=_EDGES + "the whole projected rows of the remote sources",
         bf16=("csrc/gatv2.hip", "docs/GATV2_SEMANTICS.md", "What is refused")),
    Kind("GAT", "gat", True, "attn", f"GAT with {_HEADS} (models.py:202-279)",
         unsharded=_EDGES + "the per-head scores of the remote sources"),
    Kind("GPRGNN", "gpr", True, "norm_relu", f"GPRGNN with {_NORMS} (docs/GPR_SEMANTICS.md)", unsharded=_STEPS),
    Kind("DAGNN", "dagnn", True, "norm_relu", f"DAGNN with {_NORMS} (docs/DAGNN_SEMANTICS.md)",
         unsharded=_STEPS + ", and its gate the whole propagated row", bf16=("csrc/dagnn.hip", "docs/DAGNN_SEMANTICS.md", "Out of scope"),
         stand_ins=("APPNP",), global_alone=True),
    Kind("GraphTransformer", "gt", True, "attn", f"GraphTransformer with {_HEADS} (docs/GT_SEMANTICS.md)",
         unsharded=_EDGES + "the key and value rows of the remote sources", bf16=("csrc/gt.hip", "docs/GT_SEMANTICS.md", "What is refused"),
         stand_ins=("GATv2", "GAT")),
    Kind("PNA", "pna", True, "stack", "PNA with norm_type none and ReLU (docs/PNA_SEMANTICS.md)",
         unsharded="the min, max and std of a row need every in-edge of it and each conv layer " + _LAYERS,
         bf16=("csrc/pna.hip", "docs/PNA_SEMANTICS.md", "What is refused"), stand_ins=("GCN",), global_alone=True),
)
BY_KIND = {row.kind: row for row in KINDS}
BY_KEY = {row.key: row for row in KINDS}
FULL_GRAPH_KINDS = tuple(row.kind for row in KINDS if row.full_graph)


def teacher_kind(model_name):
    """The model family a `model_name` selects: the kind of the first row of KINDS whose key the name contains (the reference's substring
    dispatch, models.py:355,409).  The order of the rows is the rule and is written down there alone: a key stands in front of every key
    it contains ("GCNII" before "GCN", "GATv2" before "GAT"; "APPNP" holds "PNP", not "PNA"), and "MLP" first ("MLP3w4" is an MLP).
    Every caller switches on the kind it returns.  The keys, in order: """
    for row in KINDS:
        if row.key in model_name:
            return row.kind
    raise ValueError(f"Unknown model_name {model_name}")


teacher_kind.__doc__ = (teacher_kind.__doc__ or "") + ", ".join(row.key for row in KINDS) + "."


def teacher_names(last, graph_kinds=False):
    """"A, B, .. <last> Z" over the full-graph teachers' keys (graph_kinds: every family with a TeacherEngine step, SAGE too), in table
    order; last="," gives the plain comma list."""
    keys = [row.key for row in KINDS if row.full_graph or (graph_kinds and row.rule)]
    return ", ".join(keys) if last == "," else ", ".join(keys[:-1]) + f" {last} " + keys[-1]
