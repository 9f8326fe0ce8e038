function [res, w, gain, cov] = gnsscorr_null_steer(hList, hDst, settings, nTaps, ref, firstSample0, nSamples, loading, targetRms)
%GNSSCORR_NULL_STEER  Wide-band interference out of the records of an antenna array, on the GPU.
%   [res, w, gain, cov] = gnsscorr_null_steer(hList, hDst, settings, nTaps, ref, firstSample0, nSamples, loading, targetRms)
%   takes the records of the K contexts hList (one device, one format), measures their covariance with one 'array_covariance'
%   command, computes the power-inversion weights for the reference element ref (1-based) over nTaps taps per element, and writes the
%   weighted sum conj(w) applied to the records into the record of context hDst (any format) from its sample 0 by 'array_combine'.
%     nTaps      default 1.     ref  default 1.     firstSample0  default 0.
%     nSamples   [] is not taken: the caller names the range (every record and hDst must hold it).
%     loading    default 0: added to the covariance's diagonal, in its units (squared counts summed over the range).
%     targetRms  [] (default): gain 1.  Else the rms a stored component should have: a trial on the first min(nSamples, 65536)
%                outputs, the weights scaled by targetRms / the rms sumSq gives, then the whole range.
%   res: clipped, sumSq, nOutputs.  w: K*nTaps x 1 complex, entry (a - 1) * nTaps + k for element a, tap k, before the gain.
%   cov: what 'array_covariance' returned.  The covariance of the stacked snapshot is taken block-Toeplitz from the lags (the
%   range-shift approximation: edge terms of at most nTaps - 1 samples).  The reference tap is tap 1, so the delay is 0: sample
%   indices, samplingFreq and IF of settings hold for hDst's record.  The same steps as receiver.null_steer of the Python package.
%   Written for this repository; not a copy of any reference file.
if nargin < 4 || isempty(nTaps), nTaps = 1; end
if nargin < 5 || isempty(ref), ref = 1; end
if nargin < 6 || isempty(firstSample0), firstSample0 = 0; end
if nargin < 8 || isempty(loading), loading = 0; end
if nargin < 9, targetRms = []; end
K = numel(hList);
T = nTaps;
cov = gnsscorr_mex('array_covariance', hList, firstSample0, nSamples, T);
c = double(cov(:));                                                            % [re; im] of C(l, a, b) at 2 * (b + K * (a + K * l)) + 1, 0-based l, a, b
R = zeros(K * T, K * T);
for a = 0:K-1
    for s = 0:T-1
        for b = 0:K-1
            for t = 0:T-1
                if t >= s
                    i = 2 * (b + K * (a + K * (t - s))) + 1;
                    v = c(i) + 1i * c(i + 1);
                else
                    i = 2 * (a + K * (b + K * (s - t))) + 1;
                    v = c(i) - 1i * c(i + 1);
                end
                R(a * T + s + 1, b * T + t + 1) = v;
            end
        end
    end
end
e = zeros(K * T, 1);
e((ref - 1) * T + 1) = 1;
u = (R + loading * eye(K * T)) \ e;
w = u / u((ref - 1) * T + 1);
wc = conj(w);
weights = [real(wc.'); imag(wc.')];                                             % 2 x (K T): re; im of element a, tap k at column (a - 1) T + k
gain = 1;
if ~isempty(targetRms)
    r = gnsscorr_mex('array_combine', hList, hDst, weights, firstSample0, min(nSamples, 65536), 0);
    components = 1 + (settings.fileType == 2);
    rmsNow = sqrt(r(2) / (components * r(3)));
    if ~(rmsNow > 0)
        error('gnsscorr:usage', 'gnsscorr_null_steer: the records hold nothing to scale');
    end
    gain = targetRms / rmsNow;
end
r = gnsscorr_mex('array_combine', hList, hDst, gain * weights, firstSample0, nSamples, 0);
res = struct('clipped', r(1), 'sumSq', r(2), 'nOutputs', r(3));
end
