"""bourse_amd: many-book limit-order-book step simulator for AMD MI355X (gfx950).

Drop-in for the ``bourse_de::Env::step`` hot path of zombie-einstein/bourse: thousands of
independent books stepped in lockstep by hand-written HIP kernels (one wavefront per book)
behind a C ABI (include/bourse_amd.h).  See DESIGN.md / INTEGRATION.md.
"""
from . import _lib, core, data_processing, step_sim
from .compat import install_as_bourse, uninstall_bourse_alias
from ._lib import (ACCOUNT_DTYPE, ACTION_MODIFY, AGENT_DESC_DTYPE, OPEN_ORDER_DTYPE, OPEN_QUEUE_DTYPE, OPEN_SUMMARY_DTYPE, QUOTE_DTYPE, QUOTE_KEEP, RANDOM_AGENTS_DTYPE, SERIES_DTYPE, TRADE_BAR_DTYPE, BourseError,
                   CapacityError, NoDeviceError, series_moments, LAG_DTYPE, lag_moments, BINS_CONFIG_DTYPE, bin_edges, bin_quantiles,
                   FLOW_DTYPE, flow_dtype, flow_moments, DEPTH_FIELDS, DEPTH_HEADER_FIELDS, depth_moments,
                   CANDLE_FIELDS, CANDLE_DTYPE, candle_series, CROSS_FIELDS, CROSS_DTYPE, CROSS_CONFIG_DTYPE, cross_moments)
from .env import (MAX_PRICE, ManyBookEnv, ManyMarketEnv, MomentumAgent, MomentumParams, NoiseAgent, NoiseAgentParams,
                  RandomAgents, RandomMarketAgents, market_sim_runner, sim_runner)

__all__ = ["core", "step_sim", "data_processing", "install_as_bourse", "uninstall_bourse_alias", "ManyBookEnv", "RandomAgents", "NoiseAgent", "NoiseAgentParams", "MomentumAgent",
           "MomentumParams", "sim_runner", "ManyMarketEnv", "RandomMarketAgents", "market_sim_runner", "MAX_PRICE", "BourseError",
           "CapacityError", "NoDeviceError", "RANDOM_AGENTS_DTYPE", "AGENT_DESC_DTYPE", "ACCOUNT_DTYPE", "OPEN_SUMMARY_DTYPE",
           "OPEN_ORDER_DTYPE", "OPEN_QUEUE_DTYPE", "QUOTE_DTYPE", "QUOTE_KEEP", "TRADE_BAR_DTYPE", "SERIES_DTYPE",
           "series_moments", "LAG_DTYPE", "lag_moments", "BINS_CONFIG_DTYPE", "bin_edges", "bin_quantiles",
           "FLOW_DTYPE", "flow_dtype", "flow_moments", "DEPTH_FIELDS", "DEPTH_HEADER_FIELDS", "depth_moments",
           "CANDLE_FIELDS", "CANDLE_DTYPE", "candle_series", "CROSS_FIELDS", "CROSS_DTYPE", "CROSS_CONFIG_DTYPE", "cross_moments"]
