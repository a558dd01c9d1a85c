"""swraytracing_amd — MI355X-native wave-packet ray tracing (gfx950 HIP).

The qg_flow_ray_trace hot loop of ndefilippis/SWRaytracing (ode_symplectic
over SpectralScheme / interpolate_U / grid_U / g2k / k2g) as hand-written
CDNA4 kernels behind the C ABI in include/swrt.h, with the reference's
MATLAB call surface mirrored in Python.
"""
from ._lib import Context, SwrtError, integrator_weights, load
from .integrate import (PacketEnsemble, combine_conds, combine_frames, combine_kmaps, combine_maps, combine_spectra, combine_tracks,
                        combine_transitions, trans_moments, combine_recycles, recycle_flux,
                        combine_refrs, alignment_edges, refr_rates,
                        combine_absfreqs, absfreq_rates, combine_tangents, tangent_growth,
                        cond_spectra, energy_spectrum, kmap_moments, map_fields,
                        ode23_packets, ode23_trajectory,
                        ode_symplectic, raytrace_sw, raytrace_xka, rsw_background, step_packet_xka)
from .io import read_field, write_field
from .qg import (QGModel, ReceiverLoop, TwoLayerLoop, flow_shells, flow_spectrum_fields, qg2layersw_raytrace,
                 qgsw_raytrace)
from .stored import read_frame, trace_stored
from .scheme import (BUMP_QG, BUMP_SW, DifferenceScheme, FourierScheme, RaytracingScheme, SnapshotPairScheme,
                     SpectralScheme, g2k, grid_U, interpolate, interpolate_U, k2g)

__all__ = [
    "Context", "SwrtError", "integrator_weights", "load", "PacketEnsemble", "combine_frames", "combine_maps", "combine_spectra",
    "combine_tracks", "combine_kmaps", "combine_conds", "cond_spectra",
    "combine_transitions", "trans_moments", "combine_recycles", "recycle_flux",
    "combine_refrs", "alignment_edges", "refr_rates",
    "combine_absfreqs", "absfreq_rates", "combine_tangents", "tangent_growth",
    "energy_spectrum", "kmap_moments", "map_fields", "ode23_packets", "ode23_trajectory",
    "ode_symplectic",
    "raytrace_sw", "raytrace_xka", "rsw_background", "step_packet_xka",
    "flow_shells", "flow_spectrum_fields", "read_field", "write_field", "QGModel", "ReceiverLoop", "TwoLayerLoop", "qgsw_raytrace", "qg2layersw_raytrace",
    "BUMP_QG", "BUMP_SW", "DifferenceScheme", "FourierScheme", "RaytracingScheme", "SnapshotPairScheme",
    "SpectralScheme", "g2k", "grid_U", "interpolate", "interpolate_U", "k2g", "read_frame", "trace_stored",
]
