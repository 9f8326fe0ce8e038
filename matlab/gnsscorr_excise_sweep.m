function res = gnsscorr_excise_sweep(h, settings, skip, nSamples, nfft, factor, widen, trainSegments, hDst)
%GNSSCORR_EXCISE_SWEEP  Swept interference (a chirp jammer) taken out of a record on the GPU, before acquisition.
%   res = gnsscorr_excise_sweep(h, settings, skip, nSamples, nfft, factor, widen, trainSegments, hDst)
%   works on the samples skip .. skip + nSamples - 1 (0-based) of the record of context h, into hDst's record (same size and
%   format; default h: in place).  In every half-overlapping segment of nfft samples (default 64) the bins whose power stands over
%   a limit, and widen (default 1) bins either side of them, are cut ('excise_sweep' of the gateway, gc_excise_sweep).
%     limit   trained on the first trainSegments (default 4096) segments of the range: a call with limit = Inf (nothing is cut)
%             gives their power; limit(b) = single(factor * median over the segments / log(2)), factor default 6 - the median of a
%             noise bin's power is log(2) times its mean, and a jammer that visits a bin a small share of the time barely moves it.
%             With hDst == h the training call works in place: a call that cuts nothing writes the record's own bytes back.
%   res: holder, limit, stats ([segments hot cut segmentsCut mostCut]), binCut (segments in which each bin was cut).
%   The same rule as receiver.excise_swept of the Python package.
%   Written for this repository; not a copy of any reference file.
if nargin < 5 || isempty(nfft), nfft = 64; end
if nargin < 6 || isempty(factor), factor = 6; end
if nargin < 7 || isempty(widen), widen = 1; end
if nargin < 8 || isempty(trainSegments), trainSegments = 4096; end
if nargin < 9 || isempty(hDst), hDst = h; end
if trainSegments < 1
    error('gnsscorr:usage', 'gnsscorr_excise_sweep: trainSegments must be at least 1');
end
nTrain = min(nSamples, trainSegments * nfft / 2);                               % segments 1 .. trainSegments lie in these samples
[st, binCut, v, power] = gnsscorr_mex('excise_sweep', h, hDst, skip, nTrain, Inf(1, nfft), 0);
rows = min(trainSegments, size(power, 2));
limit = single(factor * median(double(power(:, 1:rows)), 2) / log(2));
[st, binCut] = gnsscorr_mex('excise_sweep', h, hDst, skip, nSamples, limit, widen);
res = struct('holder', hDst, 'limit', limit, 'stats', st, 'binCut', binCut);
end
