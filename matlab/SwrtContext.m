classdef SwrtContext < handle
    % One library context (swrt_mex('create')) owned by reference: value
    % objects that hold it (SpectralSchemeGPU, and its copies) share one
    % SwrtContext, and MATLAB calls delete — which destroys the context and
    % frees its device memory (field slots, packets, streams) — when the last
    % reference goes away.  release() closes it early for every holder; a
    % later call through any copy then fails with "closed context".
    properties (SetAccess = private)
        h = 0       % swrt_mex handle; 0 once closed
    end
    methods
        function obj = SwrtContext(device)
            if nargin < 1, device = 0; end
            obj.h = swrt_mex('create', device);
        end

        function h = id(obj)
            if obj.h == 0
                error('swrt:state', 'closed context');
            end
            h = obj.h;
        end

        function release(obj)
            if obj.h ~= 0
                swrt_mex('destroy', obj.h);
                obj.h = 0;
            end
        end

        function delete(obj)
            obj.release();
        end

        % The energy-vs-omega series of the device-resident packets
        % (analysis/load_data.m:33-52,63) and the ideal distribution
        % (ideal_omega_distribution.m:3-11): thin calls into swrt_mex.
        function omega_series_begin(obj, f, Cg, edges)
            swrt_mex('omega_series_begin', obj.id(), f, Cg, edges);
        end

        function omega_series_record(obj)
            swrt_mex('omega_series_record', obj.id());
        end

        function omega_series_record_history(obj, first, count)
            % history frames first .. first+count-1, 0-based
            swrt_mex('omega_series_record_history', obj.id(), first, count);
        end

        function [counts, stats] = omega_series_get(obj)
            % counts: (nbins+2) x frames [below; bins; above]; stats: 4 x frames [n; sum; min; max]
            [counts, stats] = swrt_mex('omega_series_get', obj.id());
        end

        function omega_series_reset(obj)
            swrt_mex('omega_series_reset', obj.id());
        end

        function counts = omega_ideal(obj, slot, ring, omega0, edges)
            counts = swrt_mex('omega_ideal', obj.id(), slot, ring, omega0, edges);
        end

        % The packet density and wave-energy maps of the device-resident
        % packets (what generate_image.m:9-34 scatters packet by packet):
        % m x m cells over the periodic square of side L, integer sums of
        % the moments quantised to 2^-frac_bits.
        function map_series_begin(obj, L, m, f, Cg, frac_bits)
            if nargin < 6, frac_bits = 20; end
            swrt_mex('map_series_begin', obj.id(), L, m, f, Cg, frac_bits);
        end

        function map_series_record(obj)
            swrt_mex('map_series_record', obj.id());
        end

        function map_series_record_history(obj, first, count)
            % history frames first .. first+count-1, 0-based
            swrt_mex('map_series_record_history', obj.id(), first, count);
        end

        function [planes, stats] = map_series_get(obj)
            % planes: m x m x 4 x frames [count, sum q(omega), sum q(k), sum q(l)], first index x;
            % stats: 2 x frames [n; rejected]
            [planes, stats] = swrt_mex('map_series_get', obj.id());
        end

        function map_series_reset(obj)
            swrt_mex('map_series_reset', obj.id());
        end
    end
end
