function [x, k, t] = ode_symplectic_gpu(x0, k0, dt, T, f, gH, scheme, method)
% Drop-in for ode_symplectic (ode_symplectic.m:1-31): same arguments, same
% Nsteps x 2 x P outputs.  With a SpectralSchemeGPU the whole time loop is one
% fused device pass (swrt_leapfrog); any other scheme falls back to the
% reference implementation.
% method (optional, SpectralSchemeGPU only): 'leapfrog' (default: the
% reference's step, first order), 'midpoint' (implicit-midpoint kick, second
% order), 'yoshida4' or 'suzuki4' (fourth order) — swrt_set_integrator; the
% context's setting is restored afterwards.
    if nargin < 8
        method = 'leapfrog';
    end
    if ~isa(scheme, 'SpectralSchemeGPU')
        if ~strcmp(method, 'leapfrog')
            error('swrt:arg', 'method ''%s'' needs a SpectralSchemeGPU', method);
        end
        [x, k, t] = ode_symplectic(x0, k0, dt, T, f, gH, scheme);
        return
    end
    Nsteps = floor(T / dt);
    P = size(x0, 3);
    x = zeros([Nsteps, 2, P]);
    k = zeros([Nsteps, 2, P]);
    t = (0:Nsteps-1)' * dt;
    x(1, :, :) = x0;
    k(1, :, :) = k0;
    if Nsteps < 2
        return
    end
    X0 = reshape(x0, 2, P)';   % P x 2 (packet_x layout)
    K0 = reshape(k0, 2, P)';
    switch method  % [kick iterations composition]
        case 'leapfrog', integ = [0 1 0];
        case 'midpoint', integ = [1 2 0];
        case 'yoshida4', integ = [1 4 1];
        case 'suzuki4',  integ = [1 4 2];
        otherwise, error('swrt:arg', 'method must be leapfrog, midpoint, yoshida4 or suzuki4');
    end
    before = swrt_mex('get_integrator', scheme.h);
    swrt_mex('set_integrator', scheme.h, integ(1), integ(2), integ(3));
    restore = onCleanup(@() swrt_mex('set_integrator', scheme.h, before(1), before(2), before(3)));
    [~, ~, hx, hk] = swrt_mex('leapfrog', scheme.h, X0, K0, dt, Nsteps - 1, f, gH, 1, 0, 0, scheme.bump, 1);
    % hx: P x 2 x (Nsteps-1) frames -> Nsteps x 2 x P
    x(2:end, :, :) = permute(hx, [3 2 1]);
    k(2:end, :, :) = permute(hk, [3 2 1]);
end
