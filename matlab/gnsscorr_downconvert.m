function [res, newSettings] = gnsscorr_downconvert(h, hDst, settings, lowpass, centerFreq, decim, targetRms, nOutputs)
%GNSSCORR_DOWNCONVERT  A band of a record as a record at a lower rate, on the GPU.
%   [res, newSettings] = gnsscorr_downconvert(h, hDst, settings, lowpass, centerFreq, decim, targetRms, nOutputs)
%   takes the band around centerFreq (Hz) of the record of context h to DC and writes every decim-th filtered sample into the
%   record of context hDst (another context on the same device; any size and format), by one 'downconvert' command.
%     lowpass    the REAL low-pass of the caller, e.g. fir1(8 * decim, bandwidth / settings.samplingFreq); the wrapper moves it to
%                the band: g(k) = lowpass(k) * exp(+j 2 pi fUsed (k - 1) / fs), fUsed the frequency the NCO's 64-bit step gives
%                centerFreq.  Output m (0-based) lines up with input sample m * decim: firstSample0 = floor((T - 1) / 2).
%     targetRms  [] (default): gain 1.  Else the rms a stored component should have: the command runs on the first
%                min(nOutputs, 65536) outputs, the taps are scaled by targetRms / the rms sumSq gives, and the range runs with them.
%     nOutputs   [] (default): every output with a record sample under it, up to hDst's capacity.
%   res: clipped, sumSq, carrFreq, nOutputs.  newSettings: settings with samplingFreq / decim and IF = centerFreq - fUsed, and the
%   fields ddcGain, ddcDelay (the filter's residual delay in input samples: 0 for an odd T) and ddcDecim; a code phase found on
%   hDst's record maps back as sample * decim + ddcDelay.  The same steps as receiver.downconvert_band of the Python package.
%   Written for this repository; not a copy of any reference file.
if nargin < 7, targetRms = []; end
if nargin < 8, nOutputs = []; end
fs = settings.samplingFreq;
T = numel(lowpass);
step = round(centerFreq / fs * (2^64));                                           % whole already wherever |centerFreq / fs| >= 2^-11
fUsed = step * (2^(-64)) * fs;
ang = 2 * pi * fUsed * (0:T-1) / fs;
lp = reshape(lowpass, 1, T);
taps = [lp .* cos(ang); lp .* sin(ang)];                                       % 2 x T: re; im
first = floor((T - 1) / 2);
gain = 1;
if ~isempty(targetRms)
    if isempty(nOutputs)
        r = gnsscorr_mex('downconvert', h, hDst, taps, decim, centerFreq, 0, first);
        nTrial = min(r(4), 65536);
    else
        nTrial = min(nOutputs, 65536);
    end
    r = gnsscorr_mex('downconvert', h, hDst, taps, decim, centerFreq, 0, first, nTrial);
    components = 1 + (settings.fileType == 2);
    rmsNow = sqrt(r(2) / (components * r(4)));
    if ~(rmsNow > 0)
        error('gnsscorr:usage', 'gnsscorr_downconvert: the band holds nothing to scale');
    end
    gain = targetRms / rmsNow;
end
r = gnsscorr_mex('downconvert', h, hDst, gain * taps, decim, centerFreq, 0, first, nOutputs);
res = struct('clipped', r(1), 'sumSq', r(2), 'carrFreq', r(3), 'nOutputs', r(4));
newSettings = settings;
newSettings.samplingFreq = fs / decim;
newSettings.IF = centerFreq - fUsed;
newSettings.ddcGain = gain;
newSettings.ddcDelay = (T - 1) / 2 - first;
newSettings.ddcDecim = decim;
end
