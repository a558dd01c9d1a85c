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

        % The packet step of leapfrog / advance / advance_intervals
        % (swrt_set_integrator): kick 0 (the reference's Euler kick, first
        % order) or 1 (implicit midpoint, iterations 1..4, second order);
        % composition 0, 1 (Yoshida) or 2 (Suzuki; fourth order over kick 1).
        % method (optional, instead of the three numbers): 'leapfrog',
        % 'midpoint', 'yoshida4' or 'suzuki4'.
        function set_integrator(obj, kick, iterations, composition, method)
            if nargin > 4
                switch method
                    case 'leapfrog', kick = 0; iterations = 1; composition = 0;
                    case 'midpoint', kick = 1; iterations = 2; composition = 0;
                    case 'yoshida4', kick = 1; iterations = 4; composition = 1;
                    case 'suzuki4',  kick = 1; iterations = 4; composition = 2;
                    otherwise, error('swrt:arg', 'method must be leapfrog, midpoint, yoshida4 or suzuki4');
                end
            end
            swrt_mex('set_integrator', obj.id(), kick, iterations, composition);
        end

        function s = get_integrator(obj)
            s = swrt_mex('get_integrator', obj.id());  % [kick iterations composition]
        end

        function [w, off] = integrator_weights(~, composition)
            [w, off] = swrt_mex('integrator_weights', composition);
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

        % The conditional spectrum on the device: per frame the int64 counts
        % of the packets over omega classes (load_data.m:33-52; rows
        % [below, bins, above] over omega_edges) by the classes of a flow
        % scalar at the packets over q_edges (which 0: vorticity, 1: strain,
        % 2: Okubo-Weiss; RaytracingScheme.m:18-31), the per-class sums of
        % round(omega * 2^frac_bits), and [n; rejected].
        function cond_series_begin(obj, f, Cg, omega_edges, which, q_edges, frac_bits)
            if nargin < 7, frac_bits = 20; end
            swrt_mex('cond_series_begin', obj.id(), f, Cg, omega_edges, which, q_edges, frac_bits);
        end

        function cond_series_record(obj, nslots, alpha, bump)
            swrt_mex('cond_series_record', obj.id(), nslots, alpha, bump);
        end

        function cond_series_record_history(obj, first, count, nslots, alphas, bump)
            % history frames first .. first+count-1, 0-based; alphas [] with one snapshot
            swrt_mex('cond_series_record_history', obj.id(), first, count, nslots, alphas, bump);
        end

        function n = cond_series_frames(obj)
            n = swrt_mex('cond_series_frames', obj.id());
        end

        function [counts, sums, stats] = cond_series_get(obj)
            % counts: int64 (nw+2) x (nq+2) x frames (first index the omega class);
            % sums: int64 (nq+2) x frames; stats: int64 2 x frames
            [counts, sums, stats] = swrt_mex('cond_series_get', obj.id());
        end

        function cond_series_reset(obj)
            swrt_mex('cond_series_reset', obj.id());
        end

        % The transition series on the device: per frame the int64 counts of
        % the packets over omega classes (load_data.m:33-52; rows
        % [below, bins, above] over omega_edges) by the classes of a source
        % value kept per packet over src_edges (omega at the last mark, or
        % the values given to mark_values, e.g. the ring a packet started
        % on), per source class the sums of round(omega * 2^frac_bits),
        % round(d * ...) and round(d^2 * ...) with d = omega - source, and
        % [n; rejected; mark serial].
        function trans_series_begin(obj, f, Cg, omega_edges, src_edges, frac_bits)
            if nargin < 6, frac_bits = 20; end
            swrt_mex('trans_series_begin', obj.id(), f, Cg, omega_edges, src_edges, frac_bits);
        end

        function trans_series_mark(obj)
            swrt_mex('trans_series_mark', obj.id());
        end

        function trans_series_mark_values(obj, v)
            % one value per packet, in the order of packets_set
            swrt_mex('trans_series_mark_values', obj.id(), v);
        end

        function trans_series_record(obj)
            swrt_mex('trans_series_record', obj.id());
        end

        function trans_series_record_history(obj, first, count)
            % history frames first .. first+count-1, 0-based, against the current mark
            swrt_mex('trans_series_record_history', obj.id(), first, count);
        end

        function n = trans_series_frames(obj)
            n = swrt_mex('trans_series_frames', obj.id());
        end

        function [counts, sums, stats] = trans_series_get(obj)
            % counts: int64 (nw+2) x (ns+2) x frames (first index the omega class);
            % sums: int64 3 x (ns+2) x frames; stats: int64 3 x frames
            [counts, sums, stats] = swrt_mex('trans_series_get', obj.id());
        end

        function trans_series_reset(obj)
            swrt_mex('trans_series_reset', obj.id());
        end

        % The refraction series on the device: per frame the int64 counts of
        % the packets over omega classes (load_data.m:33-52; rows
        % [below, bins, above] over omega_edges) by the classes over a_edges
        % of the alignment c = 2 gamma / sigma of each wavevector in the
        % local strain (gamma = d ln|k|/dt from the kick's rate,
        % RaytracingScheme.m:9-16; c = 1: k on the compression axis), per
        % omega class the sums of round(omega_dot * 2^frac_bits),
        % round(omega_dot^2 * ...) and round(gamma * ...), per alignment
        % class the sum of round(omega_dot * ...), and [n; rejected].
        function refr_series_begin(obj, f, Cg, omega_edges, a_edges, frac_bits)
            if nargin < 6, frac_bits = 20; end
            swrt_mex('refr_series_begin', obj.id(), f, Cg, omega_edges, a_edges, frac_bits);
        end

        function refr_series_record(obj, nslots, alpha, bump)
            swrt_mex('refr_series_record', obj.id(), nslots, alpha, bump);
        end

        function refr_series_record_history(obj, first, count, nslots, alphas, bump)
            % history frames first .. first+count-1, 0-based; alphas [] with one snapshot
            swrt_mex('refr_series_record_history', obj.id(), first, count, nslots, alphas, bump);
        end

        function n = refr_series_frames(obj)
            n = swrt_mex('refr_series_frames', obj.id());
        end

        function [counts, sums, stats] = refr_series_get(obj)
            % counts: int64 (nw+2) x (na+2) x frames (first index the omega class);
            % sums: int64 (3(nw+2)+(na+2)) x frames; stats: int64 2 x frames
            [counts, sums, stats] = swrt_mex('refr_series_get', obj.id());
        end

        function refr_series_reset(obj)
            swrt_mex('refr_series_reset', obj.id());
        end

        % The absolute-frequency series on the device: per frame the int64
        % counts of the packets over omega classes (load_data.m:33-52; rows
        % [below, bins, above] over omega_edges) by the classes over abs_edges
        % of the absolute frequency Omega = omega + U.k
        % (symplectic_full_fourier.m:41), per omega class the sums of
        % round(Omega_dot * 2^frac_bits), round(Omega_dot^2 * ...) and
        % round(U.k * ...), per Omega class the sums of round(Omega_dot * ...)
        % and round(Omega_dot^2 * ...), and [n; rejected].  Omega_dot =
        % k.(U_b - U_a)/tau from the snapshots in slot_a (alpha = 0) and
        % slot_b (alpha = 1), 0-based; slot_b = -1: one snapshot, zero rates.
        function absfreq_series_begin(obj, f, Cg, omega_edges, abs_edges, frac_bits)
            if nargin < 6, frac_bits = 20; end
            swrt_mex('absfreq_series_begin', obj.id(), f, Cg, omega_edges, abs_edges, frac_bits);
        end

        function absfreq_series_record(obj, slot_a, slot_b, alpha, tau, bump)
            swrt_mex('absfreq_series_record', obj.id(), slot_a, slot_b, alpha, tau, bump);
        end

        function absfreq_series_record_history(obj, first, count, slot_a, slot_b, alphas, tau, bump)
            % history frames first .. first+count-1, 0-based; alphas [] with one snapshot
            swrt_mex('absfreq_series_record_history', obj.id(), first, count, slot_a, slot_b, alphas, tau, bump);
        end

        function n = absfreq_series_frames(obj)
            n = swrt_mex('absfreq_series_frames', obj.id());
        end

        function [counts, sums, stats] = absfreq_series_get(obj)
            % counts: int64 (nw+2) x (no+2) x frames (first index the omega class);
            % sums: int64 (3(nw+2)+2(no+2)) x frames; stats: int64 2 x frames
            [counts, sums, stats] = swrt_mex('absfreq_series_get', obj.id());
        end

        function absfreq_series_reset(obj)
            swrt_mex('absfreq_series_reset', obj.id());
        end

        % The ray-tube tangent map on the device: tangent_begin starts
        % carrying, per packet, M = d(x, y, k, l)/d(x0, y0, k0, l0) of the
        % discrete leapfrog step since the last mark (4 x 4, I at a mark) and
        % a caustic counter (sign changes of J = M11*M22 - M12*M21); while it
        % is live advance / leapfrog take the per-packet route (x and k keep
        % their bits) and the ode23, xka, spectral and recycle calls are
        % refused.  The series: counts of the packets over the classes of
        % s = |M|_F^2/4 (growth_edges) by omega classes, per omega class the
        % sums of floor(log2 s), floor(log2 |J|) and the counters, per growth
        % class the sum of the counters, and [n; rejected; mark serial].
        function tangent_begin(obj)
            swrt_mex('tangent_begin', obj.id());
        end

        function tangent_mark(obj)
            swrt_mex('tangent_mark', obj.id());
        end

        function [M, caustics] = tangent_get(obj)
            % M: 16 x n, column i packet i's M row-major (reshape(M(:, i), 4, 4).');
            % caustics: int64 n x 1; both in the order of packets_set
            [M, caustics] = swrt_mex('tangent_get', obj.id());
        end

        function tangent_end(obj)
            swrt_mex('tangent_end', obj.id());
        end

        function tangent_series_begin(obj, f, Cg, omega_edges, growth_edges)
            swrt_mex('tangent_series_begin', obj.id(), f, Cg, omega_edges, growth_edges);
        end

        function tangent_series_record(obj)
            swrt_mex('tangent_series_record', obj.id());
        end

        function n = tangent_series_frames(obj)
            n = swrt_mex('tangent_series_frames', obj.id());
        end

        function [counts, sums, stats] = tangent_series_get(obj)
            % counts: int64 (nw+2) x (ns+2) x frames (first index the omega class);
            % sums: int64 (3(nw+2)+(ns+2)) x frames; stats: int64 3 x frames
            [counts, sums, stats] = swrt_mex('tangent_series_get', obj.id());
        end

        function tangent_series_reset(obj)
            swrt_mex('tangent_series_reset', obj.id());
        end

        % Packet recycling on the device: at every recycle_apply a packet
        % whose omega has reached omega_cut is absorbed and re-injected in
        % place with its home wavevector (home_k, n x 2 in the order of
        % packets_set; []: the packets' k at begin) and a fresh uniform
        % position in [-L/2, L/2)^2 from a hash of (seed, index_base + its
        % index, its generation).  Per event one int64 frame [n; absorbed;
        % rejected; sum round(omega_out * 2^frac_bits); sum round(omega_home
        % * 2^frac_bits); sum age; max age; serial].
        function recycle_begin(obj, f, Cg, omega_cut, L, seed, index_base, frac_bits, home_k)
            if nargin < 6, seed = 0; end
            if nargin < 7, index_base = 0; end
            if nargin < 8, frac_bits = 20; end
            if nargin < 9, home_k = []; end
            swrt_mex('recycle_begin', obj.id(), f, Cg, omega_cut, L, seed, index_base, frac_bits, home_k);
        end

        function recycle_apply(obj)
            swrt_mex('recycle_apply', obj.id());
        end

        function n = recycle_frames(obj)
            n = swrt_mex('recycle_frames', obj.id());
        end

        function stats = recycle_get(obj)
            % int64 8 x frames
            stats = swrt_mex('recycle_get', obj.id());
        end

        function [gen, born] = recycle_state(obj)
            % int64 n x 1 each, in the order of packets_set
            [gen, born] = swrt_mex('recycle_state', obj.id());
        end

        function recycle_reset(obj)
            % frames dropped, serial and gen and born back to 0; home stays
            swrt_mex('recycle_reset', obj.id());
        end

        function recycle_end(obj)
            swrt_mex('recycle_end', obj.id());
        end

        % The wave-vector plane on the device (what raytracing_figures.m:19-26,
        % 76-83 scatter packet by packet): per frame an m x m int64 count
        % plane over [-K, K) x [-K, K), first index k, and eight int64 stats
        % [n; rejected; outside; sum q(k); sum q(l); sum q(k*k); sum q(l*l);
        % sum q(k*l)], q = round(v * 2^frac_bits).
        function kmap_series_begin(obj, K, m, frac_bits)
            if nargin < 4, frac_bits = 16; end
            swrt_mex('kmap_series_begin', obj.id(), K, m, frac_bits);
        end

        function kmap_series_record(obj)
            swrt_mex('kmap_series_record', obj.id());
        end

        function kmap_series_record_history(obj, first, count)
            % history frames first .. first+count-1, 0-based
            swrt_mex('kmap_series_record_history', obj.id(), first, count);
        end

        function n = kmap_series_frames(obj)
            n = swrt_mex('kmap_series_frames', obj.id());
        end

        function [planes, stats] = kmap_series_get(obj)
            % planes: int64 m x m x frames; stats: int64 8 x frames
            [planes, stats] = swrt_mex('kmap_series_get', obj.id());
        end

        function kmap_series_reset(obj)
            swrt_mex('kmap_series_reset', obj.id());
        end

        % The trajectories of chosen packets on the device (what
        % raytracing_figures.m:76-83 and load_data.m:29-33 take per packet,
        % for m of an ensemble too large to download): a frame is m x 8,
        % row j packet ids(j), columns [x y k l Omega zeta sigma D].
        function track_begin(obj, ids)
            % ids: original packet indices, 0-based as in the C ABI, distinct
            swrt_mex('track_begin', obj.id(), double(ids));
        end

        function track_record(obj, f, gH, nslots, alpha, bump)
            % nslots 0: no flow is read, columns 5..8 are NaN
            if nargin < 4, nslots = 1; end
            if nargin < 5, alpha = 0; end
            if nargin < 6, bump = 1e-13; end
            swrt_mex('track_record', obj.id(), f, gH, nslots, alpha, bump);
        end

        function track_record_history(obj, first, count, f, gH, nslots, alphas, bump)
            % history frames first .. first+count-1, 0-based; alphas: one per frame, [] when nslots < 2
            if nargin < 7, alphas = []; end
            if nargin < 8, bump = 1e-13; end
            swrt_mex('track_record_history', obj.id(), first, count, f, gH, nslots, alphas, bump);
        end

        function frames = track_get(obj)
            % frames: m x 8 x frames
            frames = swrt_mex('track_get', obj.id());
        end

        function track_reset(obj)
            swrt_mex('track_reset', obj.id());
        end

        % The background flow's shell spectra on the device (what
        % scratch/energy_spectrum.m:3-13 computes from a PV frame): per frame
        % nshell x 3 [E Z Q] (kinetic energy, relative-vorticity enstrophy, PV
        % variance per shell j = floor(K + .5), each half the domain mean in
        % total) and four stats [t; sum E; sum Z; sum Q].
        function flow_spectrum_begin(obj, nx, k_scale, K_d2)
            % k_scale = 2*pi/L (exactly 1 for the one-layer model)
            swrt_mex('flow_spectrum_begin', obj.id(), nx, k_scale, K_d2);
        end

        function flow_spectrum_record_qg(obj, layer)
            % the QG state's committed qk, layer 0-based
            if nargin < 2, layer = 0; end
            swrt_mex('flow_spectrum_record_qg', obj.id(), layer);
        end

        function flow_spectrum_record_qk(obj, qk, t)
            % qk: complex (2kmax+1) x (kmax+1), g2k's half plane
            if nargin < 3, t = 0; end
            swrt_mex('flow_spectrum_record_qk', obj.id(), complex(qk), t);
        end

        function n = flow_spectrum_frames(obj)
            n = swrt_mex('flow_spectrum_frames', obj.id());
        end

        function n = flow_spectrum_shells(obj)
            n = swrt_mex('flow_spectrum_shells', obj.id());
        end

        function [spectra, stats] = flow_spectrum_get(obj)
            % spectra: nshell x 3 x frames; stats: 4 x frames
            [spectra, stats] = swrt_mex('flow_spectrum_get', obj.id());
        end

        function flow_spectrum_reset(obj)
            swrt_mex('flow_spectrum_reset', obj.id());
        end
    end
end
