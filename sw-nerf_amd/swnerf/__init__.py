"""swnerf - MI355X-native NeRF volumetric renderer behind the Python call surface of
daihangpku/SW-NeRF (get_rays / ndc_rays / sample_pdf / raw2outputs / Embedder /
NeRF MLPs / run_network / render_rays / render).  See DESIGN.md and INTEGRATION.md.
Training loops: runner.train / train_dnerf / train_tnerf / train_multires (their data side: batching.RayBatcher, PatchBatcher,
photometric_loss, multires_loss) and fit2d.train."""
from . import synth  # noqa: F401  (numpy only)

__all__ = ["synth", "ray", "embedder", "model", "render", "pyramid", "runner", "fit2d", "batching"]
