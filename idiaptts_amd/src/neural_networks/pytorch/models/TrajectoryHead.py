"""TrajectoryHead: what trajectory (minimum generation error) training adds behind an acoustic model while it trains --
two `idiaptts_amd.nn.MLPGLayer`s on the model's data dictionary,

    pred_acoustic_features -> pred_trajectory        the MLPG trajectory of the prediction (differentiable)
    acoustic_features      -> acoustic_static        the target cut down to the same columns (select_only)

so that a NamedLoss can compare the two.  The layers hold corpus statistics (variances, mean, std_dev) as buffers and no
parameters; the statistics come from the data reader, not from a checkpoint.  So the head is not a child of the model:
`attach(model)` registers it as a forward hook.  The model keeps its parameters, its state-dict keys and its
`config.json`, a checkpoint written with the head attached is the checkpoint of the model alone and loads without it
(and the other way round), and constructing the head draws nothing from torch's RNG.  The hook runs on `model(...)` --
the handler's training and validation passes; `model.inference(...)` (benchmark, synthesis) calls `forward` directly
and computes no trajectory: post-processing does that there."""
from torch import nn

from .NamedForwardWrapper import NamedForwardWrapper


class TrajectoryHead(nn.Module):

    def __init__(self, layer_config, target_layer_config, batch_first, prediction_name="pred_acoustic_features",
                 target_name="acoustic_features", trajectory_name="pred_trajectory", static_name="acoustic_static"):
        super().__init__()
        self.trajectory = NamedForwardWrapper(NamedForwardWrapper.Config(
            layer_config, [prediction_name], batch_first, name="trajectory", output_names=[trajectory_name]))
        self.trajectory.reads_module_outputs = True          # (a computed tensor: nobody vouches for its padding rows)
        self.static = NamedForwardWrapper(NamedForwardWrapper.Config(
            target_layer_config, [target_name], batch_first, name="static", output_names=[static_name]))

    def forward(self, data, lengths, max_lengths):
        self.trajectory(data, lengths, max_lengths)
        self.static(data, lengths, max_lengths)
        return data

    def attach(self, model):
        """Runs the head behind every `model(data, lengths, max_lengths)` call; returns the hook's handle."""
        def run_head(module, args, output):
            self(*args[:3])
        return model.register_forward_hook(run_head)
