function res = gnsscorr_excise(h, settings, skip, nSamples, pulseSigmas, guardUs, binFactor, nfft, widen, hDst)
%GNSSCORR_EXCISE  Interference the receiver does not know taken out of a record on the GPU, before acquisition.
%   res = gnsscorr_excise(h, settings, skip, nSamples, pulseSigmas, guardUs, binFactor, nfft, widen, hDst)
%   works on the samples skip .. skip + nSamples - 1 (0-based) of the record of context h, into hDst's record (same size and
%   format; default h: in place): pulses first (pulseSigmas not []), then carriers (binFactor not []), from what the probe shows.
%     pulses  threshold2 = (pulseSigmas * sigma)^2 * components with sigma = 1.4826 * median(|first value of each pair|) from
%             'probe_histogram'; guardUs = [before after] in microseconds at settings.samplingFreq (default [4 4], at most 4096
%             samples each).  A median in the histogram's end bin is an error.
%     bins    gain 0 on the bins of 'probe_psd' (Hamming window, nfft (default 4096), overlap nfft/2, over the range after
%             blanking) above binFactor * the median bin and on widen (default 1) neighbours each side, 1 elsewhere.
%   res: holder, threshold2, sigma, before, after, stats ([hot blanked runs longest]), gain, psdBefore, psdAfter ([] for a stage
%   that did not run).  The same two rules as receiver.excise_interference of the Python package.
%   Written for this repository; not a copy of any reference file.
if nargin < 6 || isempty(guardUs), guardUs = [4 4]; end
if nargin < 7, binFactor = []; end
if nargin < 8 || isempty(nfft), nfft = 4096; end
if nargin < 9 || isempty(widen), widen = 1; end
if nargin < 10 || isempty(hDst), hDst = h; end
if isempty(pulseSigmas) && isempty(binFactor)
    error('gnsscorr:usage', 'gnsscorr_excise: give pulseSigmas, binFactor or both');
end
fs = settings.samplingFreq;
res = struct('holder', h, 'threshold2', [], 'sigma', [], 'before', [], 'after', [], 'stats', [], 'gain', [], 'psdBefore', [], 'psdAfter', []);
if ~isempty(pulseSigmas)
    counts = double(gnsscorr_mex('probe_histogram', h, skip, nSamples));        % 257 x 2: values -128 .. 128 of both components
    mag = counts(129:257, 1);                                                   % |v| = 0 .. 128 of the first component
    mag(2:end) = mag(2:end) + counts(128:-1:1, 1);
    total = sum(mag);
    cum = cumsum(mag);
    lo = find(cum >= floor((total + 1) / 2), 1) - 1;                            % the middle sample(s)
    hi = find(cum >= floor(total / 2) + 1, 1) - 1;
    if hi >= 128
        error('gnsscorr:usage', 'gnsscorr_excise: the median level lies in the histogram''s end bin (|c0| >= 128)');
    end
    res.sigma = 1.4826 * 0.5 * (lo + hi);
    components = 1 + (settings.fileType == 2);
    res.threshold2 = floor((pulseSigmas * res.sigma)^2 * components);
    res.before = min(4096, round(guardUs(1) * 1e-6 * fs));
    res.after = min(4096, round(guardUs(2) * 1e-6 * fs));
    res.stats = gnsscorr_mex('excise_pulses', h, hDst, skip, nSamples, res.threshold2, res.before, res.after);
    res.holder = hDst;
end
if ~isempty(binFactor)
    src = res.holder;                                                           % after blanking: in place on what holds it
    P = gnsscorr_mex('probe_psd', src, skip, nSamples, nfft, nfft / 2, 'hamming');
    res.psdBefore = P(:, 1);
    hot = res.psdBefore > binFactor * median(res.psdBefore);
    out = hot;
    for k = 1:widen
        out = out | circshift(hot, k) | circshift(hot, -k);                     % around the ends: bin nfft is next to bin 1
    end
    res.gain = single(~out);
    gnsscorr_mex('excise_bins', src, hDst, skip, nSamples, res.gain);
    res.holder = hDst;
    P = gnsscorr_mex('probe_psd', hDst, skip, nSamples, nfft, nfft / 2, 'hamming');
    res.psdAfter = P(:, 1);
end
end
